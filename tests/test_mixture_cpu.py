"""Mixture models (MoG, MoP) on the host: module paths, constructor rules, the reference's RNG streams
(tests/golden/mixture_gen_init.npz, minted by make_golden_mixture.py), row subsets, resume, the C ABI's argument checks
and the absence of a CPU fallback."""
import numpy as np
import pytest

from conftest import golden, has_gpu


def test_module_paths_and_defaults():
    from prosper_amd.em.mixturemodels import MixtureModel
    from prosper_amd.em.mixturemodels.MoG import MoG
    from prosper_amd.em.mixturemodels.MoP import MoP
    m = MoG(25, 10)
    assert isinstance(m, MixtureModel)
    assert m.sigmas_sq_type == 'full' and m.to_learn == ['pies', 'W', 'sigmas_sq']
    p = MoP(25, 10)
    assert isinstance(p, MixtureModel) and np.isnan(p.A) and p.to_learn == ['pies', 'W']
    assert MoP(25, 10, A=25).A == 250            # A <= D becomes 10 D (MoP.py:20-26)
    assert MoP(25, 10, A=3).A == 250
    assert MoP(25, 10, A=26).A == 26
    with pytest.raises(NotImplementedError):
        m.inference(None, {}, {})


def test_normalize():
    from prosper_amd.em.mixturemodels.MoP import MoP
    m = MoP(4, 2, A=100)
    y = np.array([[1., 2., 3., 4.], [0., 0., 0., 0.]])
    eps = np.finfo(np.float64).eps
    np.testing.assert_array_equal(m.normalize(y), ((100 - 4) / (y.sum(1) + eps))[:, None] * y + 1)


@pytest.mark.parametrize("name", ["mog_diag", "mog_full", "mop"])
def test_generate_and_standard_init_golden(name):
    from prosper_amd.em.mixturemodels.MoG import MoG
    from prosper_amd.em.mixturemodels.MoP import MoP
    g = golden("mixture_gen_init.npz")
    D, H, N = int(g["D"]), int(g["H"]), int(g["N"])
    if name == "mop":
        model, params = MoP(D, H), {"W": g["W_gt"], "pies": g["pies_gt"]}
    elif name == "mog_diag":
        model = MoG(D, H, sigmas_sq_type="diagonal")
        params = {"W": g["W_gt"], "pies": g["pies_gt"], "sigmas_sq": np.ones((H, D)) * 0.5}
    else:
        model = MoG(D, H, sigmas_sq_type="full")
        params = {"W": g["W_gt"], "pies": g["pies_gt"], "sigmas_sq": np.array([np.eye(D) * 0.7] * H)}
    np.random.seed(int(g["seed_data"]))
    data = model.generate_data(params, N)
    np.testing.assert_array_equal(data["s"], g[name + "_s"])
    np.testing.assert_array_equal(data["y"], g[name + "_y"])          # the stream, bit for bit
    np.random.seed(int(g["seed_init"]))
    init = model.standard_init(data)
    keys = sorted(k[len(name) + 6:] for k in g if k.startswith(name + "_init_"))
    assert sorted(init) == keys
    for k in keys:
        np.testing.assert_allclose(init[k], g[name + "_init_" + k], rtol=1e-12, atol=1e-12)


def test_select_partial_data_rng_order():
    from prosper_amd.em.mixturemodels.MoP import MoP
    m = MoP(3, 2)
    y = np.arange(30.).reshape(10, 3)
    s = np.arange(10)
    assert m.select_partial_data({"partial": 0}, {"y": y}) is not None
    full = {"y": y, "s": s}
    assert m.select_partial_data({"partial": 1}, full) is full
    np.random.seed(4)
    part = m.select_partial_data({"partial": 0.35}, {"y": y, "s": s, "note": "x"})
    np.random.seed(4)
    sel = np.random.permutation(10)[:4]                 # ceil(10 * 0.35) = 4, unsorted
    np.testing.assert_array_equal(part["y"], y[sel])
    np.testing.assert_array_equal(part["s"], s[sel])
    assert part["note"] == "x"


@pytest.mark.parametrize("stored,want", [("diagonal", "full"), ("full", "diagonal"), ("full", "full")])
def test_resume_init_round_trip(tmp_path, stored, want):
    from prosper_amd.em.mixturemodels.MoG import MoG
    from prosper_amd.em.mixturemodels.MoP import MoP
    from prosper_amd.utils.datalog import StoreToH5
    D, H = 4, 3
    rng = np.random.RandomState(0)
    sig = rng.uniform(1, 2, size=(H, D)) if stored == "diagonal" else np.array([np.diag(rng.uniform(1, 2, D))] * H)
    rows = [{"W": rng.normal(size=(D, H)), "pies": np.ones(H) / H, "sigmas_sq": sig + i} for i in range(2)]
    path = str(tmp_path / "result.h5")
    h = StoreToH5(path)
    for r in rows:
        for k, v in r.items():
            h.append(k, v)
    h.close()
    p = MoG(D, H, sigmas_sq_type=want).resume_init(path)
    np.testing.assert_array_equal(p["W"], rows[-1]["W"])
    np.testing.assert_array_equal(p["pies"], rows[-1]["pies"])
    last = rows[-1]["sigmas_sq"]
    if stored == "diagonal" and want == "full":
        np.testing.assert_array_equal(p["sigmas_sq"], np.array([np.diag(v) for v in last]))
    elif stored == "full" and want == "diagonal":
        np.testing.assert_array_equal(p["sigmas_sq"], np.array([v.diagonal() for v in last]))
    else:
        np.testing.assert_array_equal(p["sigmas_sq"], last)
    q = MoP(D, H).resume_init(path)
    assert sorted(q) == ["W", "pies"]


def test_abi_rejects_bad_arguments():
    from prosper_amd import _lib
    lib = _lib.load()
    EINVAL = -1
    one = 1
    assert lib.pm_mix_scores_f64(None, 4, None, None, None, 4, None, 1.0, None, 8, 4, 2, None, None, None) == EINVAL
    assert lib.pm_mix_maha_f64(None, 4, None, None, None, 8, 4, 2, None, 2, None) == EINVAL
    assert lib.pm_mix_chol_f64(None, 4, 2, None, None, None, None, None) == EINVAL
    assert lib.pm_mix_posterior_f64(None, 2, None, 1.0, None, 8, 2, None, None, None) == EINVAL
    assert lib.pm_mix_mstats_f64(None, 4, None, 2, None, 8, 4, 2, 1, None, None, None) == EINVAL
    assert lib.pm_mix_stats_len(4, 2, 3) == -1
    assert lib.pm_mix_stats_len(4, 2, 0) == 2 + 8
    assert lib.pm_mix_stats_len(4, 2, 1) == 2 + 16
    assert lib.pm_mix_stats_len(4, 2, 2) == 2 + 8 + 32
    assert lib.pm_mix_stats_chunks(0, 4, 2, 0) == -1
    assert lib.pm_mix_mstats_work_len(1000, 4, 2, one) == lib.pm_mix_stats_chunks(1000, 4, 2, one) * 18
    assert lib.pm_version() >= 1015


@pytest.mark.skipif(has_gpu(), reason="checks the behaviour without a GPU")
def test_estep_without_gpu_raises():
    from prosper_amd import _lib
    from prosper_amd.em.mixturemodels.MoG import MoG
    from prosper_amd.em.mixturemodels.MoP import MoP
    g = golden("mixture_step_mop_nan.npz")
    m = MoP(int(g["D"]), int(g["H"]))
    with pytest.raises(_lib.HipError):
        m.E_step({"T": 1.0}, {"W": g["in_W"], "pies": g["in_pies"]}, {"y": g["y"]})
    g = golden("mixture_step_mog_diag_T1.npz")
    m = MoG(int(g["D"]), int(g["H"]), sigmas_sq_type="diagonal")
    with pytest.raises(_lib.HipError):
        m.E_step({"T": 1.0}, {"W": g["in_W"], "pies": g["in_pies"], "sigmas_sq": g["in_sigmas_sq"]}, {"y": g["y"]})
