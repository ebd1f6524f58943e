"""encode() without a device: the NumPy reference of tests/encode_reference.py against itself (from log-joints
against enumeration; the union rule on a row with a repeated candidate), the two C entries (include/prosper_hip.h:
pm_encode_f64, pm_encode_exact_mca_f64) in the header, the binding table and both library builds, their argument checks, and
the refusals of the public call, all of which come before any device call."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import encode_reference as E

EINVAL, ERANGE = -1, -2
ENTRIES = ("pm_encode_f64", "pm_encode_exact_mca_f64")
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "prosper_hip.h")


@pytest.fixture(scope="module", params=[False, True], ids=["default", "deterministic"])
def lib(request):
    from prosper_amd import _lib
    return _lib.load(det=request.param)


# ------------------------------------------------------------------------------------------------ the reference itself
def test_reference_from_log_joints_equals_enumeration():
    """BSC at (D, H) = (8, 5), H' = gamma = H: the log-joints of the model's own column layout [null ; H one-cause ; S
    multi-cause states], written in NumPy, through codes_from_lpj against the enumeration of all 2^5 states."""
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    D, H, N = 8, 5, 40
    rng = np.random.RandomState(3)
    W, pi, sigma = rng.normal(size=(D, H)), 0.3, 1.1
    Y = (rng.uniform(size=(N, H)) < pi) @ W.T + sigma * rng.normal(size=(N, D))
    m = BSC_ET(D, H, H, H)
    SM = np.asarray(m.state_matrix, dtype=np.float64)
    assert SM.shape == (2 ** H - 1 - H, H)
    cand = np.stack([rng.permutation(H) for _ in range(N)])
    lp = np.empty((N, 1 + H + SM.shape[0]))
    for n in range(N):
        states = np.zeros((lp.shape[1], H))
        states[1 + np.arange(H), np.arange(H)] = 1.0
        states[1 + H:][:, cand[n]] = SM
        k = states.sum(1)
        lp[n] = k * np.log(pi) + (H - k) * np.log(1 - pi) - 0.5 * ((Y[n][None, :] - states @ W.T) ** 2).sum(1) / sigma ** 2
    mean, prob = E.codes_from_lpj(lp, 1.0, cand, H, (1.0,), 1, 1 + H, SM)
    want_mean, want_prob = E.enum_linear(Y, W, sigma, [0., 1.], np.log([1 - pi, pi]))
    assert E.rel_err(mean, want_mean) <= 1e-12 and E.rel_err(prob, want_prob) <= 1e-12
    assert E.rel_err(prob, mean) <= 1e-15 and prob.max() <= 1.0 and prob.min() >= 0.0


def tsc_row_with_a_repeated_candidate():
    """(logpj (1, 27), cand (1, 3), table (27, 3)) of one hand-made TSC row, H = 4: positions 0 and 1 both hold latent 2,
    and the state (+1, -1, 0), which is non-zero at both, carries most of the weight."""
    table = np.array([[a, b, c] for a in (-1., 0., 1.) for b in (-1., 0., 1.) for c in (-1., 0., 1.)])
    cand = np.array([[2, 2, 1]], dtype=np.int32)
    lp = np.linspace(-3.0, -1.0, 27)[None, :].copy()
    lp[0, int(np.nonzero((table == [1., -1., 0.]).all(axis=1))[0][0])] = 2.0
    return lp, cand, table


def test_union_rule_keeps_prob_at_most_one():
    lp, cand, table = tsc_row_with_a_repeated_candidate()
    H = 4
    _, naive = E.codes_from_lpj(lp, 1.0, cand, H, (), 0, 0, table, naive=True)
    assert naive[0, 2] > 1.2, naive              # summing the positions counts the heavy state twice: the case tests something
    mean, prob = E.codes_from_lpj(lp, 1.0, cand, H, (), 0, 0, table)
    q = np.exp(lp[0] - np.log(np.exp(lp[0]).sum()))
    assert prob.max() <= 1.0 and prob.min() >= 0.0
    np.testing.assert_allclose(prob[0, 2], q[((table[:, 0] != 0) | (table[:, 1] != 0))].sum(), rtol=1e-14)
    np.testing.assert_allclose(prob[0, 1], q[table[:, 2] != 0].sum(), rtol=1e-14)
    assert prob[0, 0] == 0.0 and prob[0, 3] == 0.0
    # mean counts both positions, as reconstruct() does: the heavy state's +1 and -1 cancel
    np.testing.assert_allclose(mean[0, 2], q @ (table[:, 0] + table[:, 1]), rtol=1e-13, atol=1e-15)


# ----------------------------------------------------------------------------------------------------------------- ABI
def test_entries_exported_and_version_bumped(lib):
    from prosper_amd import _lib
    assert lib.pm_version() >= 1032 and _lib.MIN_VERSION >= 1032 and lib.pm_version() >= _lib.MIN_VERSION
    for name in ENTRIES:
        assert name in _lib.SIGNATURES
        getattr(lib, name)


def _ctype(decl):
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
        assert _lib.SIGNATURES[name] == (res, [_ctype(a) for a in found.group(2).split(",")]), name
    # pm_encode_f64 takes pm_recon_expect_f64's arguments up to S, pm_encode_exact_mca_f64 those of pm_recon_exact_mca_f64
    assert _lib.SIGNATURES["pm_encode_f64"][1][:16] == _lib.SIGNATURES["pm_recon_expect_f64"][1][:16]
    assert _lib.SIGNATURES["pm_encode_exact_mca_f64"] == _lib.SIGNATURES["pm_recon_exact_mca_f64"]


# ----------------------------------------------------------------------------------------------------- argument checks
FAKE = ctypes.c_void_p(0x1000)       # never dereferenced: every call below fails its argument check or has N == 0
ONE = (ctypes.c_double * 8)(1.0, 0, 0, 0, 0, 0, 0, 0)


def _enc(lib, **kw):
    a = dict(X=FAKE, ld=40, lse=None, a=1.0, off=None, cand=FAKE, tab=FAKE, bv=ONE, N=4, H=10, Hp=4, K=40, soff=1, nblk=1,
             moff=11, S=20, mean=FAKE, ldm=10, prob=FAKE, ldp=10)
    a.update(kw)
    return lib.pm_encode_f64(a["X"], a["ld"], a["lse"], ctypes.c_double(a["a"]), a["off"], a["cand"], a["tab"], a["bv"], a["N"],
                             a["H"], a["Hp"], a["K"], a["soff"], a["nblk"], a["moff"], a["S"], a["mean"], a["ldm"], a["prob"],
                             a["ldp"], None)


def test_encode_rejects_bad_arguments(lib):
    for kw in (dict(N=-1), dict(H=0), dict(K=0), dict(ld=39), dict(ldm=9), dict(ldp=9), dict(soff=-1), dict(nblk=-1),
               dict(moff=-1), dict(S=-1), dict(Hp=-1), dict(Hp=0),                       # S > 0 needs candidates
               dict(X=None), dict(mean=None), dict(prob=None), dict(bv=None), dict(cand=None), dict(tab=None),
               dict(lse=FAKE, a=0.5), dict(lse=FAKE, off=FAKE),                          # a given lse: a = 1, no offsets
               dict(soff=31), dict(moff=21), dict(nblk=4)):                              # blocks / table past K
        assert _enc(lib, **kw) == EINVAL, kw
    assert _enc(lib, Hp=17) == ERANGE
    assert _enc(lib, nblk=9, H=2, ldm=2, ldp=2) == ERANGE
    assert _enc(lib, K=2 ** 30, ld=2 ** 30) == ERANGE


def test_encode_no_rows_is_success_without_a_device(lib):
    assert _enc(lib, N=0) == 0
    assert _enc(lib, N=0, X=None, mean=None, prob=None, cand=None, tab=None) == 0
    assert _enc(lib, N=0, ld=39) == EINVAL              # the sizes are checked at N == 0 too


def _mca(lib, **kw):
    a = dict(Y=FAKE, ldy=8, Wrho=FAKE, N=4, D=8, H=10, E=FAKE, lde=10, work=FAKE)
    a.update(kw)
    return lib.pm_encode_exact_mca_f64(a["Y"], a["ldy"], a["Wrho"], 1. / 21, 0, -1.0, -0.1, 1.0, a["N"], a["D"], a["H"],
                                       a["E"], a["lde"], a["work"], None)


def test_encode_exact_mca_argument_checks(lib):
    for kw in (dict(N=-1), dict(H=0), dict(D=0), dict(ldy=7), dict(lde=9), dict(Y=None), dict(E=None), dict(work=None),
               dict(Wrho=None)):
        assert _mca(lib, **kw) == EINVAL, kw
    assert _mca(lib, H=33, lde=33) == ERANGE
    assert _mca(lib, D=1025, ldy=1025) == ERANGE
    assert _mca(lib, N=0) == 0 and _mca(lib, N=0, Y=None, E=None) == 0
    # the work length of the reconstruction entry covers this one: nb (1 + R max(H, 2)) with nb <= 64 rows, R <= 64 ranges
    for N, H, D in ((1, 1, 1), (64, 32, 1), (65, 13, 130), (10 ** 6, 32, 1024), (3, 6, 1)):
        assert lib.pm_recon_exact_work_len(N, H, D) >= min(N, 64) * (1 + 64 * max(H, 2))


# --------------------------------------------------------------------------------- the public call, before any device
def _models():
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    from prosper_amd.em.camodels.mca_et import MCA_ET
    from prosper_amd.em.camodels.mmca_et import MMCA_ET
    from prosper_amd.em.camodels.dsc_et import DSC_ET
    from prosper_amd.em.camodels.tsc_et import TSC_ET
    from prosper_amd.em.camodels.gsc_et import GSC
    from prosper_amd.em.mixturemodels.MoG import MoG
    from prosper_amd.em.mixturemodels.MoP import MoP
    return {"bsc": lambda: BSC_ET(6, 4, 3, 2), "mca": lambda: MCA_ET(6, 4, 3, 2), "mmca": lambda: MMCA_ET(6, 4, 3, 2),
            "dsc": lambda: DSC_ET(6, 4, 3, 2), "tsc": lambda: TSC_ET(6, 4, 3, 2), "gsc": lambda: GSC(6, 4, 3, 2),
            "mog": lambda: MoG(6, 4), "mop": lambda: MoP(6, 4)}


def test_encode_is_part_of_every_model():
    for name, mk in _models().items():
        sig = inspect.signature(type(mk()).encode)
        assert list(sig.parameters) == ["self", "model_params", "my_data", "device", "exact"], name
        assert sig.parameters["device"].default is False and sig.parameters["exact"].default is False


@pytest.mark.parametrize("name", ["dsc", "tsc", "gsc", "mog", "mop"])
@pytest.mark.parametrize("key", ["mask", "weight"])
def test_mask_and_weight_are_refused_by_model_name(name, key):
    m = _models()[name]()
    with pytest.raises(NotImplementedError, match=type(m).__name__):
        m.encode({}, {'y': np.zeros((5, 6)), key: np.ones((5, 6))})


@pytest.mark.parametrize("name", ["dsc", "tsc", "gsc"])
def test_exact_is_refused_by_name(name):
    m = _models()[name]()
    with pytest.raises(NotImplementedError, match="exact"):
        m.encode({}, {'y': np.zeros((5, 6))}, exact=True)
    with pytest.raises(NotImplementedError, match="exact"):
        m.encode({}, {'y': np.zeros((0, 6))}, exact=True)


@pytest.mark.parametrize("name", ["bsc", "mca", "mmca"])
def test_exact_with_a_mask_or_weight_is_refused_by_name(name):
    m = _models()[name]()
    for key in ("mask", "weight"):
        with pytest.raises(NotImplementedError, match="exact"):
            m.encode({}, {'y': np.zeros((5, 6)), key: np.ones((5, 6))}, exact=True)


@pytest.mark.parametrize("name", ["bsc", "mca", "mmca"])
def test_wrong_observation_records_raise_value_error(name):
    m = _models()[name]()
    y = np.zeros((5, 6))
    with pytest.raises(ValueError):
        m.encode({}, {'y': y, 'mask': np.ones((5, 5), dtype=bool)})
    with pytest.raises(ValueError):
        m.encode({}, {'y': y, 'mask': np.ones(30, dtype=bool)})
    with pytest.raises(ValueError):
        m.encode({}, {'y': y, 'weight': np.ones((4, 6))})
    with pytest.raises(ValueError):
        m.encode({}, {'y': y, 'weight': -np.ones((5, 6))})
    with pytest.raises(ValueError):
        m.encode({}, {'y': y, 'mask': np.ones((5, 6)), 'weight': np.ones((5, 6))})


def test_more_than_sixteen_candidates_raise_hip_error():
    from prosper_amd import _lib
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    with pytest.raises(_lib.HipError):
        BSC_ET(16, 40, 17, 2).encode({}, {'y': np.zeros((5, 16))})


@pytest.mark.parametrize("name", ["bsc", "mca", "mmca", "dsc", "tsc", "gsc", "mog", "mop"])
def test_no_rows_give_the_empty_pair(name):
    m = _models()[name]()
    for kw in ({}, {"exact": True} if name in ("bsc", "mca", "mmca", "mog", "mop") else {}):
        out = m.encode({}, {'y': np.zeros((0, 6))}, **kw)
        assert isinstance(out, tuple) and len(out) == 2
        for a in out:
            assert isinstance(a, np.ndarray) and a.shape == (0, 4) and a.dtype == np.float64
