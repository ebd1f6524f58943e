"""log_likelihood's C entries (include/prosper_hip.h: pm_rows_lse_work_len, pm_rows_lse_f64) exist in both library builds
and reject bad arguments before anything reaches a device."""
import ctypes

import pytest


@pytest.fixture(scope="module", params=[False, True], ids=["default", "deterministic"])
def lib(request):
    from prosper_amd import _lib
    return _lib.load(det=request.param)


def test_entries_exported(lib):
    from prosper_amd import _lib
    assert lib.pm_version() >= 1016
    for name in ("pm_rows_lse_work_len", "pm_rows_lse_f64", "pm_mix_loglik_f64"):
        assert name in _lib.SIGNATURES
        getattr(lib, name)


def test_work_len(lib):
    assert lib.pm_rows_lse_work_len(-1) == -1
    assert lib.pm_rows_lse_work_len(0) == 1
    assert lib.pm_rows_lse_work_len(1) == 1
    assert lib.pm_rows_lse_work_len(200000) <= 2048
    n = [lib.pm_rows_lse_work_len(N) for N in range(1, 5000, 37)]
    assert all(v >= 1 for v in n)


def test_rows_lse_rejects_bad_arguments(lib):
    from prosper_amd import _lib
    fake = ctypes.c_void_p(0x1000)       # never dereferenced: every call below fails its argument check
    einval = -1
    f = lib.pm_rows_lse_f64
    assert f(fake, 8, -1, 8, 1.0, None, None, fake, fake, None) == einval            # N < 0
    assert f(fake, 8, 4, 0, 1.0, None, None, fake, fake, None) == einval             # S <= 0
    assert f(fake, 7, 4, 8, 1.0, None, None, fake, fake, None) == einval             # ld < S
    assert f(None, 8, 4, 8, 1.0, None, None, fake, fake, None) == einval             # no log-joints
    assert f(fake, 8, 4, 8, 1.0, None, None, None, fake, None) == einval             # no workspace
    assert f(fake, 8, 4, 8, 1.0, None, None, fake, None, None) == einval             # no total
    with pytest.raises(_lib.HipError):
        _lib.call("pm_rows_lse_f64", fake, 7, 4, 8, 1.0, None, None, fake, fake, None)


def test_every_model_has_log_likelihood():
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    from prosper_amd.em.camodels.mca_et import MCA_ET
    from prosper_amd.em.camodels.mmca_et import MMCA_ET
    from prosper_amd.em.camodels.dsc_et import DSC_ET
    from prosper_amd.em.camodels.tsc_et import TSC_ET
    from prosper_amd.em.camodels.gsc_et import GSC
    for cls in (BSC_ET, MCA_ET, MMCA_ET, DSC_ET, TSC_ET, GSC):
        assert callable(getattr(cls, "log_likelihood"))
        assert "_loglik_terms" in vars(cls) or cls is MMCA_ET      # (MMCA runs MCA's E-step with signed W)


def test_mix_loglik_rejects_bad_arguments(lib):
    fake = ctypes.c_void_p(0x1000)
    f = lib.pm_mix_loglik_f64
    ok = dict(Y=fake, ldy=8, rs=None, Bq=None, Bl=fake, ldb=8, c=fake, coef=1.0, lp=fake, N=4, D=8, H=3, pmf=0, yoff=0.0,
              rows=fake, st=None)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["Y"], a["ldy"], a["rs"], a["Bq"], a["Bl"], a["ldb"], a["c"], a["coef"], a["lp"], a["N"], a["D"], a["H"],
                 a["pmf"], a["yoff"], a["rows"], a["st"])
    assert call(N=0) == -1
    assert call(H=0) == -1
    assert call(ldy=7) == -1
    assert call(ldb=7) == -1
    assert call(rows=None) == -1
    assert call(Bl=None) == -1
    assert call(Bq=fake, pmf=1) == -1          # the lgamma row term is MoP's: no Bq
    assert call(Bq=fake, rs=fake) == -1
