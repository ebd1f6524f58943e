"""log_likelihood(..., exact=True)'s C entries (include/prosper_hip.h: pm_loglik_exact_*) exist in both library builds, their
workspace grows at most linearly in H, and they reject bad arguments before anything reaches a device."""
import ctypes
import inspect

import pytest

EINVAL, ERANGE = -1, -2
ENTRIES = ("pm_loglik_exact_work_len", "pm_loglik_exact_lin_f64", "pm_loglik_exact_mca_f64", "pm_loglik_exact_gsc_f64")


@pytest.fixture(scope="module", params=[False, True], ids=["default", "deterministic"])
def lib(request):
    from prosper_amd import _lib
    return _lib.load(det=request.param)


def test_entries_exported(lib):
    from prosper_amd import _lib
    assert lib.pm_version() >= 1017
    assert _lib.MIN_VERSION >= 1017
    for name in ENTRIES:
        assert name in _lib.SIGNATURES
        getattr(lib, name)


def test_work_len(lib):
    f = lib.pm_loglik_exact_work_len
    assert f(-1, 4) == -1 and f(4, 0) == -1
    assert f(0, 1) >= 1
    for N in (1, 2, 7, 48, 64, 1000, 10000, 123457):
        v = [f(N, H) for H in range(1, 33)]
        assert all(x >= 1 for x in v)
        assert all(b - a == v[1] - v[0] for a, b in zip(v, v[1:]))        # affine in H
        assert f(N, 32) <= 3.2 * f(N, 10)          # BSC: 2^22 times the states, not the memory
    assert f(1, 32) < 1 << 16


FAKE = ctypes.c_void_p(0x1000)       # never dereferenced: every call below fails its argument check


def _lin(lib, **kw):
    a = dict(Y=FAKE, ldy=8, mu=None, P=FAKE, G=FAKE, logp=FAKE, values=FAKE, K=2, cst=0.0, qcoef=-0.5, N=4, D=8, H=10,
             rows=None, work=FAKE, total=FAKE)
    a.update(kw)
    return lib.pm_loglik_exact_lin_f64(a["Y"], a["ldy"], a["mu"], a["P"], a["G"], a["logp"], a["values"], a["K"], a["cst"],
                                       a["qcoef"], a["N"], a["D"], a["H"], a["rows"], a["work"], a["total"], None)


def _mca(lib, **kw):
    a = dict(Y=FAKE, ldy=8, Wrho=FAKE, N=4, D=8, H=10, work=FAKE, total=FAKE)
    a.update(kw)
    return lib.pm_loglik_exact_mca_f64(a["Y"], a["ldy"], a["Wrho"], 1. / 21, 0, -1.0, -0.1, 1.0, 0.0, a["N"], a["D"],
                                       a["H"], None, a["work"], a["total"], None)


def _gsc(lib, **kw):
    a = dict(Y=FAKE, ldy=8, P=FAKE, wdiag=FAKE, Lw=None, M=FAKE, Psi=FAKE, mu=FAKE, logp=FAKE, N=4, D=8, H=10, work=FAKE,
             total=FAKE)
    a.update(kw)
    return lib.pm_loglik_exact_gsc_f64(a["Y"], a["ldy"], a["P"], a["wdiag"], a["Lw"], a["M"], a["Psi"], a["mu"], a["logp"],
                                       0.0, a["N"], a["D"], a["H"], None, a["work"], a["total"], None)


@pytest.mark.parametrize("entry", [_lin, _mca, _gsc], ids=["lin", "mca", "gsc"])
def test_rejects_bad_arguments(lib, entry):
    assert entry(lib, N=-1) == EINVAL
    assert entry(lib, H=0) == EINVAL
    assert entry(lib, D=0) == EINVAL
    assert entry(lib, ldy=7) == EINVAL
    assert entry(lib, Y=None) == EINVAL
    assert entry(lib, work=None) == EINVAL
    assert entry(lib, total=None) == EINVAL


def test_linear_rejects_bad_pointers_and_k(lib):
    for k in ("P", "G", "logp", "values"):
        assert _lin(lib, **{k: None}) == EINVAL
    for K in (-1, 0, 1, 9):
        assert _lin(lib, K=K) == EINVAL


def test_mca_gsc_reject_null_tables(lib):
    assert _mca(lib, Wrho=None) == EINVAL
    for k in ("P", "M", "Psi", "mu", "logp"):
        assert _gsc(lib, **{k: None}) == EINVAL
    assert _gsc(lib, Lw=FAKE) == EINVAL            # at most one of wdiag and Lw


def test_bounds(lib):
    from prosper_amd import _lib
    # 2^32 states and H <= 32 for the linear models, H <= 32 for MCA / MMCA, H <= 16 for GSC: one past is PM_ERANGE
    assert _lin(lib, K=2, H=33) == ERANGE
    assert _lin(lib, K=3, H=21) == ERANGE
    assert _lin(lib, K=4, H=17) == ERANGE
    assert _lin(lib, K=8, H=11) == ERANGE
    assert _mca(lib, H=33) == ERANGE
    assert _gsc(lib, H=17) == ERANGE
    with pytest.raises(_lib.HipError):
        _lib.call("pm_loglik_exact_lin_f64", FAKE, 8, None, FAKE, FAKE, FAKE, FAKE, 2, 0.0, -0.5, 4, 8, 33, None, FAKE,
                  FAKE, None)


def test_exact_is_a_keyword_of_every_model():
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    from prosper_amd.em.camodels.mca_et import MCA_ET
    from prosper_amd.em.camodels.mmca_et import MMCA_ET
    from prosper_amd.em.camodels.dsc_et import DSC_ET
    from prosper_amd.em.camodels.tsc_et import TSC_ET
    from prosper_amd.em.camodels.gsc_et import GSC
    from prosper_amd.em.mixturemodels.MoG import MoG
    from prosper_amd.em.mixturemodels.MoP import MoP
    for cls in (BSC_ET, MCA_ET, MMCA_ET, DSC_ET, TSC_ET, GSC, MoG, MoP):
        sig = inspect.signature(cls.log_likelihood)
        assert "exact" in sig.parameters and sig.parameters["exact"].default is False
    for cls in (BSC_ET, MCA_ET, DSC_ET, TSC_ET, GSC):
        assert "_loglik_exact" in vars(cls)
