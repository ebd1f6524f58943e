"""inference(exact=True) without a device: the library version and the exported entries, pm_infer_exact_plan
against the reference's restatement on a grid, the argument codes of the plan and of the entries, the coverage of the plan's
cells by the GPU module's case tables, the public keyword and every refusal (raised with no library call made), and the
reference tests/infer_exact_reference.py itself (its top-K against a full np.lexsort, its margin check on a planted near-tie).
"""
import ctypes
import inspect

import numpy as np
import pytest

import exact_kernels_reference as R
import infer_exact_reference as IR

FAKE = ctypes.c_void_p(64)            # a non-null pointer no refused call reads


@pytest.fixture(scope="module")
def libs():
    from prosper_amd import _lib
    return _lib.load(), _lib.load(True)


def _plan(lib, kind, N, D, K, H, topK):
    out = (ctypes.c_int64 * IR.PLAN_LEN)()
    rc = lib.pm_infer_exact_plan(kind, N, D, K, H, topK, out)
    return rc, (list(out) if rc == 0 else None)


def test_version_and_entries(libs):
    from prosper_amd import _lib
    assert _lib.MIN_VERSION >= 1035
    for lib in libs:
        assert lib.pm_version() >= 1035 and lib.pm_version() >= _lib.MIN_VERSION
        for name in ("pm_infer_exact_work_len", "pm_infer_exact_plan", "pm_infer_exact_lin_f64", "pm_infer_exact_mca_f64"):
            assert name in _lib.SIGNATURES and getattr(lib, name)


def test_plan_equals_the_reference_on_a_grid(libs):
    seen = set()
    for lib in libs:
        for topK in (1, 2, 7, 10, 16):
            for N in (0, 1, 63, 64, 65, 255, 256, 257, 200000):
                for K in range(2, 9):
                    for H in range(1, 33):
                        if K ** H > 2 ** 32:
                            break
                        rc, p = _plan(lib, R.LIN, N, 5, K, H, topK)
                        assert (rc, p) == IR.infer_plan(R.LIN, N, 5, K, H, topK), (N, K, H, topK, p)
                        assert p[10] + p[11] <= lib.pm_infer_exact_work_len(N, H, topK) == IR.work_len(N, H, topK)
                        assert 1 <= p[5] <= p[4] and p[6] == min(topK, K ** H)
                        seen.add((p[4], p[5]))
                for H in range(1, 33):
                    for D in (1, 64, 65, 1024):
                        rc, p = _plan(lib, R.MCA, N, D, 0, H, topK)
                        assert (rc, p) == IR.infer_plan(R.MCA, N, D, 0, H, topK), (N, D, H, topK, p)
                        assert p[10] + p[11] <= lib.pm_infer_exact_work_len(N, H, topK)
                        seen.add((p[4], p[5]))
    for space, Rr in seen:                            # the ranges partition the space, and none is empty
        edges = [space * r // Rr for r in range(Rr + 1)]
        assert edges[0] == 0 and edges[-1] == space and all(b > a for a, b in zip(edges[:-1], edges[1:])), (space, Rr)


def test_plan_argument_codes(libs):
    out = (ctypes.c_int64 * IR.PLAN_LEN)()
    for lib in libs:
        f = lib.pm_infer_exact_plan
        assert f(R.LIN, 4, 8, 2, 10, 10, None) == R.PM_EINVAL
        for kind in (R.LIN, R.MCA):
            assert f(kind, 4, 8, 2, 10, 10, out) == R.PM_OK and f(kind, 0, 1, 2, 1, 1, out) == R.PM_OK
            assert f(kind, -1, 8, 2, 10, 10, out) == R.PM_EINVAL
            assert f(kind, 4, 0, 2, 10, 10, out) == R.PM_EINVAL
            assert f(kind, 4, 8, 2, 0, 10, out) == R.PM_EINVAL
            assert f(kind, 4, 8, 2, 10, 0, out) == R.PM_EINVAL and f(kind, 4, 8, 2, 10, -1, out) == R.PM_EINVAL
            assert f(kind, 4, 8, 2, 10, 16, out) == R.PM_OK and f(kind, 4, 8, 2, 10, 17, out) == R.PM_ERANGE
        for kind in (-1, R.GSC, 3):
            assert f(kind, 4, 8, 2, 10, 10, out) == R.PM_EINVAL
        for K in (-1, 0, 1, 9):
            assert f(R.LIN, 4, 8, K, 10, 10, out) == R.PM_EINVAL and f(R.MCA, 4, 8, K, 10, 10, out) == R.PM_OK
        for K, H in ((2, 33), (3, 21), (4, 17), (5, 14), (6, 13), (7, 12), (8, 11)):
            assert f(R.LIN, 4, 8, K, H, 10, out) == R.PM_ERANGE and f(R.LIN, 4, 8, K, H - 1, 10, out) == R.PM_OK
        assert f(R.MCA, 4, 8, 0, 33, 10, out) == R.PM_ERANGE and f(R.MCA, 4, 8, 0, 32, 10, out) == R.PM_OK
        assert f(R.MCA, 4, 1025, 0, 10, 10, out) == R.PM_ERANGE and f(R.MCA, 4, 1024, 0, 10, 10, out) == R.PM_OK
        assert f(R.LIN, 4, 1025, 2, 10, 10, out) == R.PM_OK
        assert lib.pm_infer_exact_work_len(-1, 4, 10) == -1 and lib.pm_infer_exact_work_len(4, 0, 10) == -1
        assert lib.pm_infer_exact_work_len(4, 4, 0) == -1 and lib.pm_infer_exact_work_len(4, 4, 17) == -1


def test_entries_return_the_plans_codes_without_a_device(libs):
    """Every argument the entries refuse returns the documented code before a device is touched (the pointers are fakes)."""
    out = (ctypes.c_int64 * IR.PLAN_LEN)()
    for lib in libs:
        refused = 0
        for N, D, K, H, topK in [(-1, 8, 2, 10, 10), (4, 0, 2, 10, 10), (4, 8, 2, 0, 10), (4, 8, 9, 10, 10), (4, 8, 1, 40, 10),
                                 (4, 8, 2, 33, 10), (4, 8, 3, 21, 10), (4, 8, 8, 11, 10), (4, 1025, 2, 6, 10), (4, 8, 2, 10, 0),
                                 (4, 8, 2, 10, 17)]:
            ldy = max(D, 1)
            lin = lambda: lib.pm_infer_exact_lin_f64(FAKE, ldy, None, FAKE, FAKE, FAKE, FAKE, K, N, D, H, topK, FAKE, 16, FAKE,
                                                     16, FAKE, FAKE, None)
            mca = lambda: lib.pm_infer_exact_mca_f64(FAKE, ldy, FAKE, 0.1, 0, -1.0, -0.1, 1.0, N, D, H, topK, FAKE, 16, FAKE, 16,
                                                     FAKE, FAKE, None)
            for kind, entry in ((R.LIN, lin), (R.MCA, mca)):
                want = lib.pm_infer_exact_plan(kind, N, D, K, H, topK, out)
                if want != R.PM_OK:
                    assert entry() == want, (kind, N, D, K, H, topK)
                    refused += 1
        assert refused >= 12
        # short leading dimensions and null pointers: PM_EINVAL
        assert lib.pm_infer_exact_lin_f64(FAKE, 7, None, FAKE, FAKE, FAKE, FAKE, 2, 4, 8, 10, 10, FAKE, 16, FAKE, 16, FAKE, FAKE,
                                          None) == R.PM_EINVAL
        assert lib.pm_infer_exact_lin_f64(FAKE, 8, None, FAKE, FAKE, FAKE, FAKE, 2, 4, 8, 10, 10, FAKE, 9, FAKE, 16, FAKE, FAKE,
                                          None) == R.PM_EINVAL
        assert lib.pm_infer_exact_mca_f64(FAKE, 8, FAKE, 0.1, 0, -1.0, -0.1, 1.0, 4, 8, 10, 10, FAKE, 16, FAKE, 9, FAKE, FAKE,
                                          None) == R.PM_EINVAL
        assert lib.pm_infer_exact_mca_f64(FAKE, 8, FAKE, 0.1, 0, -1.0, -0.1, 1.0, 4, 8, 10, 10, None, 16, FAKE, 16, FAKE, FAKE,
                                          None) == R.PM_EINVAL
        assert lib.pm_infer_exact_lin_f64(FAKE, 8, None, FAKE, FAKE, FAKE, FAKE, 2, 4, 8, 10, 10, FAKE, 16, FAKE, 16, FAKE, None,
                                          None) == R.PM_EINVAL
        # N == 0 launches nothing
        assert lib.pm_infer_exact_lin_f64(None, 8, None, FAKE, FAKE, FAKE, FAKE, 2, 0, 8, 10, 10, None, 16, None, 16, None, FAKE,
                                          None) == R.PM_OK
        assert lib.pm_infer_exact_mca_f64(None, 8, FAKE, 0.1, 0, -1.0, -0.1, 1.0, 0, 8, 10, 10, None, 16, None, 16, None, FAKE,
                                          None) == R.PM_OK


def test_every_plan_cell_has_a_gpu_case(libs):
    """The cells the plan reports over the grid of shapes the unit distinguishes are all cells of a case the GPU module runs;
    a new cell in the plan (another range rule, another block size) fails here until a case covers it."""
    lib = libs[0]
    lin_cells = {IR.state_cell(R.LIN, K, H, topK) for K, H, N, topK, _ in IR.LIN_CASES}
    mca_cells = {IR.state_cell(R.MCA, 0, H, topK) for _, H, N, D, topK, _ in IR.MCA_CASES}
    for K, H in IR.CELL_GRID_LIN:
        for topK in IR.CELL_TOPK:
            assert _plan(lib, R.LIN, 3, 5, K, H, topK) == IR.infer_plan(R.LIN, 3, 5, K, H, topK)
            assert IR.state_cell(R.LIN, K, H, topK) in lin_cells, (K, H, topK)
    for H in IR.CELL_GRID_MCA:
        for topK in IR.CELL_TOPK:
            assert _plan(lib, R.MCA, 3, 5, 0, H, topK) == IR.infer_plan(R.MCA, 3, 5, 0, H, topK)
            assert IR.state_cell(R.MCA, 0, H, topK) in mca_cells, (H, topK)
    for kind, cases, n_of in ((R.LIN, IR.LIN_CASES, lambda c: c[2]), (R.MCA, IR.MCA_CASES, lambda c: c[2])):
        have = {IR.walk_cell(kind, n_of(c)) for c in cases}
        for N in IR.CELL_N[kind]:
            p = _plan(lib, kind, N, 5, 2, 6, 10)[1]
            assert p[:2] == [256 if kind == R.LIN else 64, -(-N // p[0])]
            assert IR.walk_cell(kind, N) in have, (kind, N)
    # the literal cells the issue names, as the plan reports them: (L, CH, chunks, R)
    for (K, H), want in {(2, 1): (1, 2, 1, 1), (2, 3): (3, 8, 1, 1), (2, 10): (10, 1024, 1, 1), (2, 11): (10, 1024, 2, 1),
                         (2, 12): (10, 1024, 4, 2), (2, 14): (10, 1024, 16, 8), (3, 7): (6, 729, 3, 1), (3, 8): (6, 729, 9, 4),
                         (8, 4): (3, 512, 8, 4)}.items():
        assert tuple(_plan(lib, R.LIN, 3, 5, K, H, 10)[1][2:6]) == want, (K, H)
    for H, want in {1: (2, 1), 6: (64, 1), 7: (128, 2), 11: (2048, 32)}.items():
        assert tuple(_plan(lib, R.MCA, 3, 5, 0, H, 10)[1][4:6]) == want, H
    assert {c[3] for c in IR.LIN_CASES} >= set(IR.CELL_TOPK) and {c[2] for c in IR.LIN_CASES} >= set(R.LIN_RECON_N)
    assert {c[2] for c in IR.MCA_CASES} >= set(R.MCA_RECON_N) and {c[3] for c in IR.MCA_CASES} >= set(R.MCA_RECON_D)
    assert {c[1] for c in IR.MCA_CASES} >= set(R.MCA_H) and {c[4] for c in IR.MCA_CASES} >= set(IR.CELL_TOPK)


# ------------------------------------------------------------------------------------------------------- the public call
def _models():
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    from prosper_amd.em.camodels.mca_et import MCA_ET
    from prosper_amd.em.camodels.mmca_et import MMCA_ET
    from prosper_amd.em.camodels.dsc_et import DSC_ET
    from prosper_amd.em.camodels.tsc_et import TSC_ET
    from prosper_amd.em.camodels.gsc_et import GSC
    return {"bsc": BSC_ET, "mca": MCA_ET, "mmca": MMCA_ET, "dsc": DSC_ET, "tsc": TSC_ET, "gsc": GSC}


def test_exact_is_the_last_keyword_of_inference_everywhere():
    for name, cls in _models().items():
        sig = inspect.signature(cls.inference)
        assert list(sig.parameters)[-1] == "exact" and sig.parameters["exact"].default is False, name
        assert sig.parameters["topK"].default == 10 and sig.parameters["adaptive"].default is True


@pytest.fixture
def no_library_calls(monkeypatch):
    """Any call into the library through the package's two doors fails the test."""
    from prosper_amd import _lib
    from prosper_amd.em.camodels._device import DeviceCAModel

    def boom(*a, **k):
        raise AssertionError("a library call was made before the refusal")
    monkeypatch.setattr(_lib, "call", boom)
    monkeypatch.setattr(DeviceCAModel, "_call", boom)


def _params(D, H):
    rng = np.random.RandomState(0)
    return {"W": np.abs(rng.normal(size=(D, H))) + 0.5, "pi": 0.2, "sigma": 1.0}


T1 = {"T": 1.0}


@pytest.mark.parametrize("name", ["dsc", "tsc", "gsc"])
def test_other_models_refuse_exact_by_name(name, no_library_calls):
    m = _models()[name](6, 4, 3, 2)
    with pytest.raises(NotImplementedError, match=type(m).__name__) as e:
        m.inference(T1, _params(6, 4), {"y": np.zeros((5, 6))}, exact=True)
    assert "exact" in str(e.value)


@pytest.mark.parametrize("name", ["bsc", "mca", "mmca"])
def test_refusals_before_any_library_call(name, no_library_calls):
    from prosper_amd import _lib
    cls = _models()[name]
    m, par, data = cls(6, 4, 3, 2), _params(6, 4), {"y": np.zeros((5, 6))}
    with pytest.raises(NotImplementedError, match="T = 1"):
        m.inference({"T": 1.5}, par, data, exact=True)
    for kw in ({"Hprime_max": 4}, {"gamma_max": 3}, {"Hprime_max": 4, "gamma_max": 4}):
        with pytest.raises(ValueError, match="nothing to grow"):
            m.inference(T1, par, data, exact=True, **kw)
    for topK in (-1, 0, -5, 17, 1000):
        with pytest.raises(ValueError, match="topK"):
            m.inference(T1, par, data, topK=topK, exact=True)
    for key in ("mask", "weight"):
        with pytest.raises(NotImplementedError, match="exact"):
            m.inference(T1, par, dict(data, **{key: np.ones((5, 6))}), exact=True)
    big = cls(6, 33, 3, 2)
    with pytest.raises(_lib.HipError, match="H <= 32"):
        big.inference(T1, _params(6, 33), data, exact=True)
    if name != "bsc":
        wide = cls(1025, 4, 3, 2)
        with pytest.raises(_lib.HipError, match="D <= 1024"):
            wide.inference(T1, _params(1025, 4), {"y": np.zeros((2, 1025))}, exact=True)
    assert m.Hprime == 3 and m.gamma == 2


def test_mixtures_inference_is_unchanged():
    from prosper_amd.em.mixturemodels.MoG import MoG
    assert "exact" not in inspect.signature(MoG.inference).parameters


# --------------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_reference_topk_is_a_full_lexsort_on_tiny_spaces(seed):
    rng = np.random.RandomState(seed)
    for K, H in ((2, 1), (2, 3), (2, 4), (3, 3), (4, 2)):
        op = R.lin_operands(rng, 4, H, K, 6)
        l = IR.lin_table(op["Y"], op["ymu"], op["P"], op["G"], op["logp"], op["values"])
        l[0, :] = np.round(l[0, :])                      # exact ties in one row, -inf among the values already
        S = K ** H
        for topK in (1, 2, S, S + 3):
            idx, vals, v = IR.topk_rows(l, topK)
            cols = min(topK, S)
            assert idx.shape == vals.shape == (6, cols)
            for n in range(6):
                full = np.lexsort((np.arange(S), -l[n]))                # primary key -l, then the index
                assert np.array_equal(idx[n], full[:cols]) and np.array_equal(vals[n], l[n][full[:cols]])
            assert np.allclose(np.asarray(v, dtype=float), np.log(np.exp(np.asarray(l, dtype=float)).sum(axis=1)))
    for H in (1, 2, 4):
        op = R.mca_operands(rng, 5, H, 4, signed=seed % 2)
        l = IR.mca_table(op["Y"], op["Wrho"], op["inv_rho"], op["signed"], op["lp1"], op["lp0"], op["inv_s2"])
        idx, vals, _ = IR.topk_rows(l, 3)
        for n in range(4):
            assert np.array_equal(idx[n], np.lexsort((np.arange(1 << H), -l[n]))[:min(3, 1 << H)])


def test_reference_nan_row_and_margin():
    rng = np.random.RandomState(3)
    l = np.asarray(rng.normal(size=(4, 16)) * 3, dtype=IR.LD)
    assert IR.assert_margin(l, 5) > IR.MARGIN
    planted = l.copy()
    order = np.argsort(-planted[2])
    planted[2, order[4]] = planted[2, order[3]] * (1 - IR.LD(1e-10))          # a near-tie between the 4th and 5th best
    with pytest.raises(AssertionError, match="near-tie"):
        IR.assert_margin(planted, 5)
    IR.assert_margin(planted, 2)                           # ... which a shorter list does not reach
    planted[2, order[5]] = planted[2, order[4]]            # the (topK + 1)-th entry counts: it could enter the list
    with pytest.raises(AssertionError, match="near-tie"):
        IR.assert_margin(planted, 4)
    l[1, 7] = np.nan
    idx, vals, v = IR.topk_rows(l, 5)
    assert np.all(idx[1] == -1) and np.all(np.isnan(vals[1])) and np.isnan(v[1])
    assert np.all(idx[[0, 2, 3]] >= 0) and not np.isnan(np.asarray(v, dtype=float)[[0, 2, 3]]).any()


def test_planted_orders_are_pure_tie_breaking():
    ops, dist = IR.planted_lin(3, 4, 50)
    assert dist[50] == 0 and sorted(set(dist)) == [0, 1, 2, 3, 4]
    l = IR.lin_table(np.tile(ops["ymu"], (2, 1)), ops["ymu"], ops["P"], ops["G"], ops["logp"], ops["values"])
    assert np.array_equal(np.asarray(l[0], dtype=float), -dist.astype(float))
    idx, score = IR.planted_order(dist, 10)
    assert idx[0] == 50 and np.array_equal(IR.topk_rows(l, 10)[0][0], idx)
    assert np.array_equal(IR.popcounts(3), [0, 1, 1, 2, 1, 2, 2, 3])


def test_the_issues_margin_figures():
    """The random GPU cases satisfy the margin condition in the reference's own values, every row (checked again by the GPU
    module before every comparison)."""
    for K, H, N, topK, seed in IR.LIN_CASES:
        if K ** H > 2 ** 12 or N > 3:
            continue
        op = R.lin_operands(np.random.RandomState(seed), 5, H, K, N)
        IR.assert_margin(IR.lin_table(op["Y"], op["ymu"], op["P"], op["G"], op["logp"], op["values"]), topK)
