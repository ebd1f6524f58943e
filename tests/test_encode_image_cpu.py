"""encode_image() / pool_codes() without a GPU: the region rule, the plain-Python reference the GPU tests
compare against (tests/encode_image_reference.py) pinned against math.fsum and shown to see the summation order, every
argument error raised before any device call, the method on all eight models, and the pm_codes_pool_* entries in the
header, the binding and both libraries with their argument checks."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import encode_image_reference as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pm_codes_pool_work_len", "pm_codes_pool_f64", "pm_codes_pool_finish_f64")
PM_EINVAL, PM_ERANGE = -1, -2

# (B, nr, nc, gh, gw, H): the three cases whose order-sensitivity was counted, and cases with few terms per region
ORDER_CASES = [(2, 5, 7, 2, 2, 3), (3, 2, 65, 2, 1, 65), (1, 5, 129, 5, 2, 130), (1, 2, 2, 1, 2, 4), (2, 5, 7, 5, 7, 3),
               (1, 3, 8, 1, 2, 5)]


# ------------------------------------------------------------------------------------------------------- the region rule
def test_pool_regions_partition_the_axis():
    from prosper_amd.utils.patches import pool_regions
    for n in list(range(1, 40)) + [64, 65, 129, 505]:
        for g in sorted(set([1, 2, 3, n // 2, n - 1, n]) - {0}):
            if g > n:
                continue
            regions = pool_regions(n, g)
            assert regions == E.pool_regions(n, g), (n, g)
            assert len(regions) == g and regions[0][0] == 0 and regions[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(regions, regions[1:]))              # ascending, no gap, no overlap
            lengths = [stop - start for start, stop in regions]
            assert min(lengths) >= 1 and max(lengths) - min(lengths) <= 1, (n, g, lengths)
            assert all(isinstance(v, int) for r in regions for v in r)
    for n, g in ((5, 0), (5, 6), (5, -1), (1, 2), (0, 0), (5, 2.5)):
        with pytest.raises(ValueError):
            pool_regions(n, g)
    assert pool_regions(5, 2) == [(0, 2), (2, 5)] and pool_regions(7, 3) == [(0, 2), (2, 4), (4, 7)]


# ---------------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("case", ORDER_CASES)
def test_reference_sum_is_within_its_rounding_bound_of_fsum(case):
    """n - 1 rounded additions of n terms (and the one of +0, exact): |sum - fsum| <= n 2^-52 sum |x|; the mean is that sum
    divided once; the maximum is exact."""
    B, nr, nc, gh, gw, H = case
    x = E.wide_range(np.random.RandomState(0), (B * nr * nc, H))
    got = E.pool(x, (B, nr, nc), (gh, gw), "sum")
    mean = E.pool(x, (B, nr, nc), (gh, gw), "mean")
    top = E.pool(x, (B, nr, nc), (gh, gw), "max")
    X = x.reshape(B, nr, nc, H)
    worst = 0.0
    for b in range(B):
        for i, (r0, r1) in enumerate(E.pool_regions(nr, gh)):
            for j, (c0, c1) in enumerate(E.pool_regions(nc, gw)):
                block = X[b, r0:r1, c0:c1].reshape(-1, H)
                n = len(block)
                for h in range(H):
                    exact, size = math.fsum(block[:, h]), math.fsum(np.abs(block[:, h]))
                    worst = max(worst, abs(got[b, i, j, h] - exact) / (n * 2.0 ** -52 * size))
                    assert abs(got[b, i, j, h] - exact) <= n * 2.0 ** -52 * size
                    assert mean[b, i, j, h] == got[b, i, j, h] / n
                    assert top[b, i, j, h] == block[:, h].max()
    print("reference sum %r: worst |sum - fsum| = %.3f of n 2^-52 sum |x|" % (case, worst))


@pytest.mark.parametrize("case", ORDER_CASES)
def test_reference_sees_the_summation_order(case):
    """Inputs normal * 10^uniform(-8, 8): where the largest region has at least 12 terms, adding in descending instead of
    ascending order changes at least one output bit -- a kernel that adds in another order cannot pass the bit comparison."""
    B, nr, nc, gh, gw, H = case
    x = E.wide_range(np.random.RandomState(0), (B * nr * nc, H))
    fwd = E.pool(x, (B, nr, nc), (gh, gw), "sum")
    rev = E.pool(x, (B, nr, nc), (gh, gw), "sum", reverse=True)
    terms = max(r1 - r0 for r0, r1 in E.pool_regions(nr, gh)) * max(c1 - c0 for c0, c1 in E.pool_regions(nc, gw))
    differ = int((fwd.view(np.uint64) != rev.view(np.uint64)).sum())
    print("order %r: %d terms in the largest region, %d of %d outputs differ between the two orders" % (
        case, terms, differ, fwd.size))
    if terms >= 12:
        assert differ >= 1
    assert np.allclose(fwd, rev, rtol=1e-9, atol=1e-9 * np.abs(x).max())
    # the maximum does not depend on the order, zeros of either sign included
    z = np.where(np.random.RandomState(1).uniform(size=x.shape) < 0.5, 0.0, -0.0)
    for data in (x, z):
        a, b = E.pool(data, (B, nr, nc), (gh, gw), "max"), E.pool(data, (B, nr, nc), (gh, gw), "max", reverse=True)
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_reference_maximum_keeps_a_nan_and_prefers_plus_zero():
    assert math.isnan(E.larger(1.0, math.nan)) and math.isnan(E.larger(math.nan, 1.0))
    assert math.copysign(1.0, E.larger(-0.0, 0.0)) == 1.0 and math.copysign(1.0, E.larger(0.0, -0.0)) == 1.0
    assert math.copysign(1.0, E.larger(-0.0, -0.0)) == -1.0
    assert E.larger(-math.inf, -math.inf) == -math.inf and E.larger(-math.inf, -1e300) == -1e300
    x = np.array([[1.0], [math.nan], [3.0], [2.0], [5.0], [4.0]])
    out = E.pool(x, (1, 2, 3), (2, 1), "max")
    assert math.isnan(out[0, 0, 0, 0]) and out[0, 1, 0, 0] == 5.0


# ------------------------------------------------------------------------------ argument errors before any device call
class _NoDevice(object):
    """A model whose device must not be asked for and whose encode() must not see data: argument errors come first."""
    D, H = 16, 6
    deterministic = False

    def __init__(self):
        self.empty_calls = []

    @property
    def device(self):
        raise AssertionError("the device was touched before the arguments were checked")

    def encode(self, model_params, my_data, device=False, **kw):
        assert my_data['y'].shape == (0, self.D) and not device, "encode() saw data before the arguments were checked"
        self.empty_calls.append((sorted(my_data), kw))
        return np.empty((0, self.H)), np.empty((0, self.H))


def test_argument_errors_come_before_any_device_call(monkeypatch):
    from prosper_amd import _lib
    from prosper_amd.utils import patches as U

    def no_call(*a, **k):
        raise AssertionError("a device entry was called before the arguments were checked")
    monkeypatch.setattr(_lib, "call", no_call)
    monkeypatch.setattr(U, "_device", no_call)
    img = np.zeros((10, 12))                                            # p = 4, stride 1: a 7 x 9 patch grid
    m = _NoDevice()
    bad = [dict(patch=(4, 5)), dict(chunk=0), dict(chunk=2.5), dict(stride=-1), dict(stride=0), dict(stride=5),
           dict(reduce='median'), dict(reduce=None), dict(reduce='Mean'), dict(pool=2, reduce='min'),
           dict(pool=0), dict(pool=(8, 2)), dict(pool=(2, 10)), dict(pool=8), dict(pool=(2, 2, 2)), dict(pool=1.5),
           dict(pool=(2, -1)), dict(pool='2'),
           dict(mask=np.ones((10, 12)), center=True), dict(weight=np.ones((10, 12)), center=True),
           dict(mask=np.ones((10, 12)), weight=np.ones((10, 12))),
           dict(mask=np.ones((10, 11))), dict(weight=np.ones((9, 12))),
           dict(weight=-np.ones((10, 12))), dict(weight=np.full((10, 12), np.nan)), dict(weight=np.full((10, 12), np.inf))]
    for kw in bad:
        with pytest.raises(ValueError):
            U.encode_image(m, {}, img, **kw)
    assert m.empty_calls == []
    with pytest.raises(ValueError):
        U.encode_image(m, {}, np.zeros((3, 12)))                       # L < p
    with pytest.raises(ValueError):
        U.encode_image(m, {}, np.zeros((2, 3, 10, 12)))                # colour channels are out of scope
    m.D = 15
    with pytest.raises(ValueError):
        U.encode_image(m, {}, img)                                     # D is not a square and no patch is given
    m.D = 16
    # the order of denoise_image: mask with centre, weight with mask, weight with centre -- each before the shapes are read
    with pytest.raises(ValueError, match="center=True with a mask"):
        U.encode_image(m, {}, img, mask=np.ones((3, 3)), weight=np.ones((3, 3)), center=True)
    with pytest.raises(ValueError, match="together with 'mask'"):
        U.encode_image(m, {}, img, mask=np.ones((3, 3)), weight=np.ones((3, 3)))
    with pytest.raises(ValueError, match="center=True with a weight"):
        U.encode_image(m, {}, img, weight=np.ones((3, 3)), center=True)
    # a valid masked / weighted call reaches the model's empty encode() -- with exact only when it is set -- and then the device
    for key, kw, want in (("mask", {}, {}), ("weight", {}, {}), ("mask", {"exact": True}, {"exact": True})):
        m.empty_calls = []
        with pytest.raises(AssertionError, match="device entry"):
            U.encode_image(m, {}, img, pool=2, **dict(kw, **{key: np.ones((10, 12))}))
        assert m.empty_calls == [(sorted(["y", key]), want)]

    # pool_codes
    codes = np.zeros((63, 5))
    for args, kw in (((codes, (1, 7, 9), 2), dict(reduce='median')), ((codes, (1, 7, 8), 2), {}), ((codes, (7, 9), 2), {}),
                     ((codes, (1, 7, 9), 8), {}), ((codes, (1, 7, 9), (2, 10)), {}), ((codes, (1, 7, 9), 0), {}),
                     ((codes, (0, 7, 9), 1), {}), ((np.zeros(63), (1, 7, 9), 2), {}), ((np.zeros((63, 0)), (1, 7, 9), 2), {}),
                     ((codes, (1, 7, 9), (2, 2, 2)), {})):
        with pytest.raises(ValueError):
            U.pool_codes(*args, **kw)


def _classes():
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    from prosper_amd.em.camodels.mca_et import MCA_ET
    from prosper_amd.em.camodels.mmca_et import MMCA_ET
    from prosper_amd.em.camodels.dsc_et import DSC_ET
    from prosper_amd.em.camodels.tsc_et import TSC_ET
    from prosper_amd.em.camodels.gsc_et import GSC
    from prosper_amd.em.mixturemodels.MoG import MoG
    from prosper_amd.em.mixturemodels.MoP import MoP
    return BSC_ET, MCA_ET, MMCA_ET, DSC_ET, TSC_ET, GSC, MoG, MoP


def test_every_model_has_encode_image():
    import inspect
    for cls in _classes():
        assert callable(getattr(cls, "encode_image", None)), cls.__name__
        assert "utils.patches.encode_image" in cls.encode_image.__doc__, cls.__name__
        assert list(inspect.signature(cls.encode_image).parameters) == ["self", "model_params", "image", "mask", "weight", "kw"]


@pytest.mark.parametrize("index", [3, 4, 5, 6, 7])
@pytest.mark.parametrize("key", ["mask", "weight"])
def test_models_without_the_masked_estep_refuse_by_name_before_any_device_call(monkeypatch, index, key):
    from prosper_amd import _lib
    from prosper_amd.utils import patches as U

    def no_call(*a, **k):
        raise AssertionError("a device entry was called before the refusal")
    monkeypatch.setattr(_lib, "call", no_call)
    monkeypatch.setattr(U, "_device", no_call)
    cls = _classes()[index]
    m = cls(16, 6) if index >= 6 else cls(16, 6, 4, 3)
    with pytest.raises(NotImplementedError, match=cls.__name__):
        m.encode_image({}, np.zeros((10, 12)), **{key: np.ones((10, 12))})


# ----------------------------------------------------------------------------------------------------------------- ABI
def _ctype(decl):
    decl = decl.strip()
    if "*" in decl:
        return C.c_void_p
    base = decl.rsplit(None, 1)[0].replace("const", "").strip()
    return {"int64_t": C.c_int64, "int": C.c_int, "double": C.c_double}[base]


def test_new_entries_in_header_binding_and_both_libraries():
    from prosper_amd import _lib
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "prosper_hip.h")).read(), flags=re.S)
    for name in NEW:
        found = re.search(r"(int64_t|int)\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert found, "%s is not declared in prosper_hip.h" % name
        res = {"int64_t": C.c_int64, "int": C.c_int}[found.group(1)]
        assert _lib.SIGNATURES[name] == (res, [_ctype(a) for a in found.group(2).split(",")]), name
    for path in (_lib.LIB_PATH, _lib.LIB_PATH_DET):
        lib = C.CDLL(path)
        for name in NEW:
            assert hasattr(lib, name), (path, name)
    assert _lib.load().pm_version() >= 1033 and _lib.MIN_VERSION >= 1033 and _lib.load(True).pm_version() >= 1033


@pytest.mark.parametrize("det", [False, True])
def test_entries_reject_bad_arguments_without_a_device(det):
    """Every pointer below is host memory (or NULL): a launch would fault, a correct entry returns before one."""
    from prosper_amd import _lib
    lib = _lib.load(det)
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)

    def pool(codes=p, ldc=6, n0=0, n=18, B=2, nr=3, nc=9, gh=2, gw=3, H=6, mode=0, acc=p, work=p):
        return lib.pm_codes_pool_f64(codes, ldc, n0, n, B, nr, nc, gh, gw, H, mode, acc, work, None)
    assert pool(codes=None) == PM_EINVAL and pool(acc=None) == PM_EINVAL and pool(work=None) == PM_EINVAL
    for kw in (dict(B=0), dict(nr=0), dict(nc=0), dict(gh=0), dict(gw=0), dict(H=0), dict(B=-1), dict(H=-3),
               dict(gh=4), dict(gw=10), dict(ldc=5), dict(mode=2), dict(mode=-1),
               dict(n0=-9), dict(n=-9), dict(n0=45, n=18), dict(n0=54, n=9), dict(n=63),
               dict(n0=1), dict(n0=4, n=9), dict(n=10), dict(n=1)):
        assert pool(**kw) == PM_EINVAL, kw
    assert pool(nr=2 ** 30 + 1) == PM_ERANGE and pool(nc=2 ** 30 + 1, n=0) == PM_ERANGE
    assert pool(H=2 ** 20 + 1, ldc=2 ** 20 + 1) == PM_ERANGE
    assert pool(n=0) == 0 and pool(n0=54, n=0) == 0                                       # nothing to do: no launch
    assert pool(nr=2 ** 30, nc=2 ** 30, gh=2 ** 30, gw=2 ** 30, H=2 ** 20, ldc=2 ** 20, n=0) == 0    # the limits themselves

    def fin(acc=p, out=p, B=2, nr=3, nc=9, gh=2, gw=3, H=6):
        return lib.pm_codes_pool_finish_f64(acc, out, B, nr, nc, gh, gw, H, None)
    assert fin(acc=None) == PM_EINVAL and fin(out=None) == PM_EINVAL
    for kw in (dict(B=0), dict(nr=0), dict(nc=0), dict(gh=0), dict(gw=0), dict(H=0), dict(gh=4), dict(gw=10)):
        assert fin(**kw) == PM_EINVAL, kw
    assert fin(nr=2 ** 30 + 1) == PM_ERANGE and fin(nc=2 ** 30 + 1) == PM_ERANGE and fin(H=2 ** 20 + 1) == PM_ERANGE

    wl = lib.pm_codes_pool_work_len
    assert wl(18, 9, 3, 6) == 2 * 3 * 6 and wl(0, 9, 3, 6) == 0 and wl(9, 9, 9, 1) == 9 and wl(645, 129, 2, 130) == 5 * 2 * 130
    assert wl(10, 9, 3, 6) == -1 and wl(-9, 9, 3, 6) == -1 and wl(18, 9, 10, 6) == -1 and wl(18, 9, 0, 6) == -1
    assert wl(18, 0, 3, 6) == -1 and wl(18, 9, 3, 0) == -1 and wl(18, 9, 3, 2 ** 20 + 1) == -1
