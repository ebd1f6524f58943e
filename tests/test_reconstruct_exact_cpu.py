"""reconstruct(..., exact=True)'s C entries (include/prosper_hip.h: pm_recon_exact_*) exist in both library
builds with the signatures the header declares, reject bad arguments before anything reaches a device, and the keyword is
part of every model's, reconstruct_image's and denoise_image's signature; a mask together with it is refused by name."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

EINVAL, ERANGE = -1, -2
ENTRIES = ("pm_recon_exact_work_len", "pm_recon_exact_lin_f64", "pm_recon_exact_mca_f64", "pm_recon_exact_gsc_f64")
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "prosper_hip.h")


@pytest.fixture(scope="module", params=[False, True], ids=["default", "deterministic"])
def lib(request):
    from prosper_amd import _lib
    return _lib.load(det=request.param)


def test_entries_exported(lib):
    from prosper_amd import _lib
    assert lib.pm_version() >= 1023
    assert _lib.MIN_VERSION >= 1023 and lib.pm_version() >= _lib.MIN_VERSION
    for name in ENTRIES:
        assert name in _lib.SIGNATURES
        getattr(lib, name)


def _ctype(decl):
    """The ctypes type _lib.py uses for one parameter declaration of the header."""
    decl = decl.strip()
    if "*" in decl:
        return ctypes.c_void_p
    base = decl.rsplit(None, 1)[0].replace("const", "").strip()
    return {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "double": ctypes.c_double}[base]


def test_header_and_binding_table_agree():
    from prosper_amd import _lib
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    for name in ENTRIES:
        found = re.search(r"(int64_t|int)\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert found, "%s is not declared in prosper_hip.h" % name
        res = {"int64_t": ctypes.c_int64, "int": ctypes.c_int}[found.group(1)]
        args = [_ctype(a) for a in found.group(2).split(",")]
        assert _lib.SIGNATURES[name] == (res, args), name


def test_work_len(lib):
    f = lib.pm_recon_exact_work_len
    assert f(-1, 4, 4) == -1 and f(4, 0, 4) == -1 and f(4, 4, 0) == -1
    assert f(0, 1, 1) >= 1
    # bounded in N (the entries walk N in row blocks of a fixed size): the same from one block on
    for H, D in ((6, 20), (32, 20), (10, 1024)):
        assert f(256, H, D) == f(257, H, D) == f(10 ** 7, H, D)
        assert 1 <= f(1, H, D) <= f(64, H, D) <= f(256, H, D)
    # ... and in the state count: at most linear in H, whatever 2^H is
    assert f(10 ** 7, 32, 20) <= 3.3 * f(10 ** 7, 10, 20)
    assert f(10 ** 7, 32, 1024) * 8 < 1 << 27


FAKE = ctypes.c_void_p(0x1000)       # never dereferenced: every call below fails its argument check or has N == 0


def _lin(lib, **kw):
    a = dict(Y=FAKE, ldy=8, mu=None, P=FAKE, G=FAKE, logp=FAKE, values=FAKE, K=2, N=4, D=8, H=10, E=FAKE, lde=10, work=FAKE)
    a.update(kw)
    return lib.pm_recon_exact_lin_f64(a["Y"], a["ldy"], a["mu"], a["P"], a["G"], a["logp"], a["values"], a["K"], a["N"],
                                      a["D"], a["H"], a["E"], a["lde"], a["work"], None)


def _mca(lib, **kw):
    a = dict(Y=FAKE, ldy=8, Wrho=FAKE, N=4, D=8, H=10, E=FAKE, lde=8, work=FAKE)
    a.update(kw)
    return lib.pm_recon_exact_mca_f64(a["Y"], a["ldy"], a["Wrho"], 1. / 21, 0, -1.0, -0.1, 1.0, a["N"], a["D"], a["H"],
                                      a["E"], a["lde"], a["work"], None)


def _gsc(lib, **kw):
    a = dict(Y=FAKE, ldy=8, P=FAKE, M=FAKE, Psi=FAKE, mu=FAKE, logp=FAKE, N=4, D=8, H=10, E=FAKE, lde=10, work=FAKE)
    a.update(kw)
    return lib.pm_recon_exact_gsc_f64(a["Y"], a["ldy"], a["P"], a["M"], a["Psi"], a["mu"], a["logp"], a["N"], a["D"], a["H"],
                                      a["E"], a["lde"], a["work"], None)


@pytest.mark.parametrize("entry", [_lin, _mca, _gsc], ids=["lin", "mca", "gsc"])
def test_rejects_bad_arguments(lib, entry):
    assert entry(lib, N=-1) == EINVAL
    assert entry(lib, H=0) == EINVAL
    assert entry(lib, D=0) == EINVAL
    assert entry(lib, ldy=7) == EINVAL                       # ldy < D
    assert entry(lib, lde=7) == EINVAL                       # the output's leading dimension below its row width
    assert entry(lib, Y=None) == EINVAL
    assert entry(lib, E=None) == EINVAL
    assert entry(lib, work=None) == EINVAL


def test_rejects_null_tables_and_bad_k(lib):
    for k in ("P", "G", "logp", "values"):
        assert _lin(lib, **{k: None}) == EINVAL
    for K in (-1, 0, 1, 9):
        assert _lin(lib, K=K) == EINVAL
    assert _mca(lib, Wrho=None) == EINVAL
    for k in ("P", "M", "Psi", "mu", "logp"):
        assert _gsc(lib, **{k: None}) == EINVAL


def test_bounds(lib):
    from prosper_amd import _lib
    assert _lin(lib, K=2, H=33, lde=33) == ERANGE
    assert _lin(lib, K=3, H=21, lde=21) == ERANGE            # 3^21 > 2^32
    assert _lin(lib, K=4, H=17, lde=17) == ERANGE
    assert _lin(lib, K=8, H=11, lde=11) == ERANGE
    assert _mca(lib, H=33) == ERANGE
    assert _mca(lib, D=1025, ldy=1025, lde=1025) == ERANGE
    assert _gsc(lib, H=17, lde=17) == ERANGE
    with pytest.raises(_lib.HipError):
        _lib.call("pm_recon_exact_lin_f64", FAKE, 8, None, FAKE, FAKE, FAKE, FAKE, 2, 4, 8, 33, FAKE, 33, FAKE, None)


@pytest.mark.parametrize("entry", [_lin, _mca, _gsc], ids=["lin", "mca", "gsc"])
def test_no_rows_is_success_without_a_device(lib, entry):
    assert entry(lib, N=0) == 0
    assert entry(lib, N=0, Y=None, E=None) == 0


def _models():
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    from prosper_amd.em.camodels.mca_et import MCA_ET
    from prosper_amd.em.camodels.mmca_et import MMCA_ET
    from prosper_amd.em.camodels.dsc_et import DSC_ET
    from prosper_amd.em.camodels.tsc_et import TSC_ET
    from prosper_amd.em.camodels.gsc_et import GSC
    from prosper_amd.em.mixturemodels.MoG import MoG
    from prosper_amd.em.mixturemodels.MoP import MoP
    return BSC_ET, MCA_ET, MMCA_ET, DSC_ET, TSC_ET, GSC, MoG, MoP


def test_exact_is_a_keyword_of_every_model():
    for cls in _models():
        sig = inspect.signature(cls.reconstruct)
        assert "exact" in sig.parameters and sig.parameters["exact"].default is False, cls
        assert list(sig.parameters)[:4] == ["self", "model_params", "my_data", "device"], cls
        assert hasattr(cls, "reconstruct_image")


def test_denoise_image_takes_exact():
    from prosper_amd.utils import patches
    sig = inspect.signature(patches.denoise_image)
    assert "exact" in sig.parameters and sig.parameters["exact"].default is False


@pytest.mark.parametrize("name", ["bsc", "mca"])
def test_mask_with_exact_is_refused_by_name(name):
    BSC_ET, MCA_ET = _models()[:2]
    m = (BSC_ET if name == "bsc" else MCA_ET)(6, 4, 3, 2)
    y = np.zeros((5, 6))
    with pytest.raises(NotImplementedError, match="exact"):
        m.reconstruct({}, {'y': y, 'mask': np.ones((5, 6), dtype=bool)}, exact=True)
    with pytest.raises(NotImplementedError, match="exact"):
        m.reconstruct({}, {'y': np.zeros((0, 6)), 'mask': np.ones((0, 6), dtype=bool)}, exact=True)
    with pytest.raises(NotImplementedError, match="exact"):
        m.reconstruct_image({}, np.zeros((4, 4)), mask=np.ones((4, 4), dtype=bool), patch=(2, 3), exact=True)
