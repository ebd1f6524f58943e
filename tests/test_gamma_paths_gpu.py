"""gamma > 4 on every dispatch path, and the reference's shipped truncation settings (examples/barstests/param-bars-*.py:
BSC / MCA H' = 8, MMCA / DSC / TSC H' = 7 at gamma = 5, GSC H' = 7 at gamma = 4).

(a) The 30-step runs of tests/golden/shipped_traj_<model>.npz (the param files' own schedules, minted from the reference by
    tests/golden/make_golden.py::shipped_traj) through the drop-in ``EM(...).run()``, on the fast path and with the next E-step
    launch and the deferred statistics off.
(b) The plain-NumPy oracle (oracle/*_oracle.py, vec flavour) against each code path the host layer can pick at gamma >= 5: every
    case asserts which kernels ran (the names passed to ``_call``, the ``_fused`` / ``_state_tables`` switches, the
    ``pm_*_supported`` predicates), and compares candidates (equal), log-joints (1e-10) and one whole ``step`` (the tolerances
    of the model's own ``test_*_step_matches_oracle``).  The seeds have no selection near-ties: candidates are asserted equal."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


class _An(dict):
    crit_params = []

    def __missing__(self, k):
        return 0.0

    def as_dict(self):
        return dict(self)


def _spy(m):
    """Names of the library entries the model calls from now on."""
    names = []
    orig = m._call
    m._call = lambda label, name, *a: (names.append(name), orig(label, name, *a))[1]
    return names


def _cp(p):
    return {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in p.items()}


def _logged(fn, names=("L", "N_use")):
    from prosper_amd.utils.datalog import dlog, StoreInMemory
    h = dlog.set_handler(names, StoreInMemory)
    try:
        out = fn()
    finally:
        dlog.remove_handler(h)
    return out, h.tables


# ------------------------------------------------------------------------------------------------ (a) shipped schedules
SHIPPED = ("bsc", "mca", "mmca", "dsc", "tsc", "gsc")
# per-step tolerance on the parameters, relative to the largest entry: those of test_schedule_golden_gpu.py for the same model
# (a trajectory is a discontinuous map of its inputs -- candidate selection, the cut -- so rounding-level differences grow)
TRAJ_TOL = {"bsc": 1e-11, "gsc": 1e-9, "mca": 1e-7, "mmca": 1e-7, "dsc": 1e-9, "tsc": 1e-9}


def _shipped_model(kind, z):
    D, H, Hp, g = (int(z[k]) for k in ("D", "H", "Hprime", "gamma"))
    if kind == "bsc":
        from prosper_amd.em.camodels.bsc_et import BSC_ET
        return BSC_ET(D, H, Hp, g)
    if kind == "mca":
        from prosper_amd.em.camodels.mca_et import MCA_ET
        return MCA_ET(D, H, Hp, g)
    if kind == "mmca":
        from prosper_amd.em.camodels.mmca_et import MMCA_ET
        return MMCA_ET(D, H, Hp, g)
    if kind == "dsc":
        from prosper_amd.em.camodels.dsc_et import DSC_ET
        return DSC_ET(D, H, Hp, g, states=np.array(z["states"]))
    if kind == "tsc":
        from prosper_amd.em.camodels.tsc_et import TSC_ET
        return TSC_ET(D, H, Hp, g)
    from prosper_amd.em.camodels.gsc_et import GSC
    return GSC(D, H, Hp, g, "scalar")


@pytest.mark.parametrize("fast", [True, False])
@pytest.mark.parametrize("kind", SHIPPED)
def test_shipped_schedule_follows_the_reference(kind, fast):
    from prosper_amd.em import EM
    from prosper_amd.em.annealing import LinearAnnealing
    z = np.load(os.path.join(GOLDEN, "shipped_traj_%s.npz" % kind))
    steps = int(z["steps"])
    m = _shipped_model(kind, z)
    assert (m.Hprime, m.gamma) == ((7, 4) if kind == "gsc" else (8, 5) if kind in ("bsc", "mca") else (7, 5))
    if not fast:
        m.speculate_estep = False
        if hasattr(m, "defer_stats"):
            m.defer_stats = False
    pnames = [k[:-1] for k in z.files if k.endswith("0") and k[:-1] in z.files]
    an = LinearAnnealing(steps)
    an["T"] = [tuple(float(v) for v in r) for r in z["T_points"]]
    an["Ncut_factor"] = [tuple(float(v) for v in r) for r in z["Ncut_points"]]
    an["anneal_prior"] = False
    em = EM(model=m, anneal=an, data={"y": z["y"]}, lparams={k: np.array(z[k + "0"], copy=True) for k in pnames})
    _, got = _logged(em.run, tuple(pnames) + ("L", "N_use"))
    if len(z["N_use"]) == steps:
        np.testing.assert_array_equal(np.array(got["N_use"], dtype=np.int64), z["N_use"].astype(np.int64))
        assert z["N_use"][-1] < z["N"]                       # (the schedule does reach the truncation steps)
    if len(z["L"]) == steps:
        np.testing.assert_allclose(np.array(got["L"], dtype=float), z["L"], rtol=1e-10)
    tol = TRAJ_TOL[kind]
    for k in pnames:
        a, ref = np.array([np.asarray(v, dtype=float) for v in got[k]]), z[k]
        assert a.shape == ref.shape, k
        for t in range(steps):
            dev = float(np.abs(a[t] - ref[t]).max() / max(np.abs(ref[t]).max(), 1e-300))
            assert dev <= tol, "%s after step %d: %.2e of its largest entry" % (k, t, dev)


# ------------------------------------------------------------------------------------------------ (b) BSC
def _bsc_problem(D, H, N, seed):
    """(sigma = 2 at D = 1024: the oracle's un-stabilised exp(logpj) sums -- the reference's -- stay above the underflow
    threshold, as for the config-2 goldens)"""
    from oracle import bsc_oracle as O
    rng = np.random.RandomState(seed)
    W_gt = rng.normal(size=(D, H))
    sig = 2.0 if D >= 1024 else 1.0
    y, _ = O.generate_bsc_data(W_gt, 2.5 / H, sig, N, rng)
    return y, {"W": W_gt + 0.2 * rng.normal(size=(D, H)), "pi": 2.5 / H * 1.2, "sigma": 1.1 * sig}


def _bsc_vs_oracle(D, H, Hp, gamma, N, seed, path, T=1.0, ncut=0.0, expect=None):
    """select_Hprimes -> E_step on the chosen path against the oracle, then one ``step`` of a fresh model on the same path."""
    from oracle import bsc_oracle as O
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    y, params = _bsc_problem(D, H, N, seed)
    ref, rlog = O.em_step(O.Anneal(T=T, Ncut_factor=ncut, anneal_prior=False), O.make_model(D, H, Hp, gamma), _cp(params), y,
                          stats_fn=O.m_step_stats_vec, vec=True)

    def make():
        m = BSC_ET(D, H, Hp, gamma)
        m.use_rows16 = path != "wave64"
        m.use_fused = path == "fused"
        assert m._state_tables()["fast"] == (path != "wave64"), "the 16-lane tables do not apply at this shape"
        assert m._fused() == (path == "fused"), "the one-kernel pass does not apply at this shape"
        return m
    m = make()
    an = _An(T=T, Ncut_factor=ncut, anneal_prior=False)
    p = _cp(params)
    data = m.select_Hprimes(p, {"y": y})
    ss = m.E_step(an, p, data)
    assert np.array_equal(np.asarray(data["candidates"]).astype(np.int64), rlog["candidates"])
    np.testing.assert_allclose(np.asarray(ss["logpj"]), rlog["logpj"], rtol=1e-10, atol=1e-9)
    m = make()
    names = _spy(m)
    new, log = _logged(lambda: m.step(an, _cp(params), {"y": y}))
    assert int(log["N_use"][0]) == rlog["N_use"]
    # (at D = 1024 every log-joint is ~2e3 and carries the scores GEMM's rounding up to the 1e-10 bound held above; their mean
    # -- L -- inherits up to twice that: measured 1.4e-10 at (1024, 200, 8, 5))
    np.testing.assert_allclose(float(log["L"][0]), rlog["L"], rtol=1e-10 if D < 1024 else 2e-10)
    tol = max(1e-8, 20 * np.linalg.cond(rlog["stats"]["Wq"]) * np.finfo(float).eps)
    np.testing.assert_allclose(new["W"], ref["W"], rtol=10 * tol, atol=tol * np.abs(ref["W"]).max())
    np.testing.assert_allclose(new["pi"], ref["pi"], rtol=1e-9)
    np.testing.assert_allclose(new["sigma"], ref["sigma"], rtol=1e-9)
    for name in expect or ():
        assert name in names, (name, sorted(set(names)))
    return m, names


@pytest.mark.parametrize("D,H,Hp,gamma,N,path,ncut,expect", [
    (64, 40, 8, 5, 500, "fused", 0.0, ("pm_bsc_estep_fused_f64",)),            # 4-wavefront one-kernel pass (H <= 256)
    (64, 40, 8, 5, 500, "fused", 0.6, ("pm_bsc_estep_fused_f64", "pm_kth_round_k_f64")),    # ... a truncation step
    (64, 40, 8, 5, 500, "rows16", 0.0, ("pm_gemm_nt_f64", "pm_bsc_select_estep_f64")),        # scores GEMM + 16-lane rows
    (64, 40, 8, 5, 500, "wave64", 0.0, ("pm_bsc_select_f64", "pm_bsc_estep_f64")),          # generic kernels
    (48, 24, 8, 8, 300, "fused", 0.0, ("pm_bsc_estep_fused_f64",)),            # gamma = H' = 8: 247 multi-cause states
    (48, 24, 8, 8, 300, "rows16", 0.4, ()),
    (48, 600, 8, 5, 300, "wave64", 0.0, ("pm_bsc_select_f64", "pm_bsc_estep_f64")),        # H > 512: generic only
])
def test_bsc_gamma5_paths_match_oracle(D, H, Hp, gamma, N, path, ncut, expect):
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    if H > 512:
        assert not BSC_ET(D, H, Hp, gamma)._state_tables()["fast"]
    _bsc_vs_oracle(D, H, Hp, gamma, N, D + H + N, path, T=1.2, ncut=ncut, expect=expect)


def test_bsc_state_set_beyond_the_16_lane_lds():
    """(12, 5): 1573 multi-cause states -- more than the 16-lane row kernels keep in LDS: the generic kernels take the shape
    on their own, and agree with the oracle."""
    from prosper_amd import _lib
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    m = BSC_ET(64, 40, 12, 5)
    assert m.no_states == 1573 and not _lib.load().pm_bsc_rows16_supported(40, 12, 1573)
    assert not m._state_tables()["fast"] and not m._fused()
    _bsc_vs_oracle(64, 40, 12, 5, 200, 7, "wave64", expect=("pm_bsc_select_f64", "pm_bsc_estep_f64"))


@pytest.mark.parametrize("H", [256, 200])
def test_bsc_config2_shape_gamma5_fused_round_and_ragged_rest(H):
    """D = 1024, (8, 5) at N = 40 000.  H = 256 (config 2): the one-kernel pass does not hold 210 states there
    (pm_bsc_fused_supported), the two-kernel path runs.  H = 200: whole rounds of the one-kernel pass plus the ragged rest on
    the two-kernel path, with the M-step statistics fused into the pass, and on a truncation step.  Against
    the two-kernel path, which the oracle pins at N = 600 first."""
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    D, Hp, gamma = 1024, 8, 5
    fusable = H == 200
    assert BSC_ET(D, H, Hp, gamma)._fused() == fusable
    _bsc_vs_oracle(D, H, Hp, gamma, 600, 3, "rows16", T=1.1)
    if fusable:
        _bsc_vs_oracle(D, H, Hp, gamma, 600, 3, "fused", T=1.1)
    N = 40000
    y, params = _bsc_problem(D, H, N, 4)
    for ncut in (0.0, 0.6):
        out = {}
        for mode in ("fused_ms", "fused", "two_kernel") if fusable else ("fused_ms", "two_kernel"):
            m = BSC_ET(D, H, Hp, gamma)
            m.fuse_mstats = mode == "fused_ms"
            m.use_fused = mode != "two_kernel"
            on = fusable and mode != "two_kernel"
            assert m._fused() == on
            if on:
                assert 0 < m._fused_rows(N) < N                  # a whole round of the kernel, and a ragged rest behind it
            names = _spy(m)
            new, log = _logged(lambda: m.step(_An(T=1.1, Ncut_factor=ncut), _cp(params), {"y": y}))
            out[mode] = (new, float(log["L"][0]), int(log["N_use"][0]))
            assert ("pm_bsc_estep_fused_f64" in names) == on and "pm_gemm_nt_f64" in names, sorted(set(names))
            if ncut:
                # (the deferred per-datapoint records belong to the 16-wavefront tile, gamma in {3, 4}: at gamma = 5 the M-step
                # runs its own statistics pass behind the cut)
                assert "pm_bsc_defer_apply_f64" not in names and "pm_kth_round_k_f64" in names, sorted(set(names))
        b = out["two_kernel"]
        for mode in sorted(set(out) - {"two_kernel"}):
            a = out[mode]
            assert a[2] == b[2] and (a[2] < N) == bool(ncut)
            np.testing.assert_allclose(a[1], b[1], rtol=1e-12)
            for k in ("W", "pi", "sigma"):
                np.testing.assert_allclose(a[0][k], b[0][k], rtol=1e-8, atol=1e-10)


# ------------------------------------------------------------------------------------------------ (b) MCA / MMCA
def _mca_problem(cls_name, D, H, N, seed):
    rng = np.random.RandomState(seed)
    if cls_name == "MCA_ET":
        from oracle import mca_oracle as M
        W_gt = np.abs(rng.normal(size=(D, H))) * 2.0 + 0.1
        y, _ = M.generate_mca_data(W_gt, 2.0 / H, 1.0, N, rng)
        jit = 0.2
    else:
        from oracle import mmca_oracle as M
        W_gt = rng.normal(size=(D, H)) * 3.0
        y = M.generate_from_hidden(W_gt, rng.random_sample((N, H)) < 2.0 / H) + rng.normal(size=(N, D))
        jit = 0.2 if D < 200 else 0.02 if D < 600 else 0.005
    return M, y, {"W": W_gt * (1 + jit * rng.uniform(-1, 1, size=(D, H))), "pi": 2.4 / H, "sigma": 1.1}


def _mca_vs_oracle(cls_name, D, H, Hp, gamma, N, seed, T=1.0, ncut=0.0, fuse=True):
    import importlib
    mod = importlib.import_module("prosper_amd.em.camodels." + ("mca_et" if cls_name == "MCA_ET" else "mmca_et"))
    cls = getattr(mod, cls_name)
    M, y, params = _mca_problem(cls_name, D, H, N, seed)
    m = cls(D, H, Hp, gamma)
    m.fuse_em = fuse
    p = m.check_params(_cp(params))
    model = M.make_model(D, H, Hp, gamma)
    ref, rlog = M.em_step(M.Anneal(T=T, Ncut_factor=ncut), model, _cp(p), y, vec=True)
    data = m.select_Hprimes(p, {"y": y})
    ss = m.E_step(_An(T=T, Ncut_factor=ncut), p, data)
    assert np.array_equal(np.asarray(data["candidates"]).astype(np.int64), rlog["candidates"])
    np.testing.assert_allclose(np.asarray(ss["logpj"]), rlog["logpj"], rtol=1e-10, atol=1e-9)
    m = cls(D, H, Hp, gamma)
    m.fuse_em = fuse
    names = _spy(m)
    new, log = _logged(lambda: m.step(_An(T=T, Ncut_factor=ncut), _cp(p), {"y": y}), ("N_use",))
    assert int(log["N_use"][0]) == rlog["N_use"]
    np.testing.assert_allclose(new["W"], ref["W"], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(new["pi"], ref["pi"], rtol=1e-9)
    np.testing.assert_allclose(new["sigma"], ref["sigma"], rtol=1e-9)
    if np.isfinite(ref["Q"]):       # (else the reference's un-stabilised log-evidence underflowed: DESIGN.md, test_mca_gpu.py)
        np.testing.assert_allclose(new["Q"], ref["Q"], rtol=1e-10)
    return names, new


@pytest.mark.parametrize("cls_name", ["MCA_ET", "MMCA_ET"])
@pytest.mark.parametrize("D,H,Hp,gamma,N,ncut", [
    (40, 24, 8, 5, 300, 0.0), (100, 24, 8, 5, 300, 0.0), (200, 24, 8, 5, 200, 0.0),        # the E-step's D buckets
    (400, 24, 8, 5, 150, 0.0), (1000, 24, 8, 5, 90, 0.0),                                 # (<= 64, 128, 256, 512, 1024)
    (60, 40, 12, 5, 120, 0.0), (60, 40, 16, 5, 60, 0.0),                                  # the M-step's 12- / 16-wide tiles
    (100, 24, 8, 5, 257, 0.5),                                                           # a truncation step
])
def test_mca_gamma5_matches_oracle(cls_name, D, H, Hp, gamma, N, ncut):
    names, _ = _mca_vs_oracle(cls_name, D, H, Hp, gamma, N, D + H + N + Hp, T=1.2, ncut=ncut)
    fused = "pm_mca_estep_mstats_defer_f64" in names
    # (the fused E+M pass covers D <= 512 and H' <= 12 with a small enough tile; beyond: E-step + M-step rows kernels)
    hp_tile = 4 if Hp <= 4 else 8 if Hp <= 8 else 12
    dpl = 1 if D <= 64 else 2 if D <= 128 else 4 if D <= 256 else 8
    assert fused == (D <= 512 and Hp <= 12 and dpl * hp_tile <= 48), sorted(set(names))
    if not fused:
        assert "pm_mca_estep_f64" in names and "pm_mca_mstep_rows_f64" in names, sorted(set(names))


@pytest.mark.parametrize("cls_name", ["MCA_ET", "MMCA_ET"])
def test_mca_gamma5_fused_pass_matches_two_passes(cls_name):
    a, na = _mca_vs_oracle(cls_name, 100, 30, 8, 5, 400, 17, T=1.3, fuse=True)
    b, nb = _mca_vs_oracle(cls_name, 100, 30, 8, 5, 400, 17, T=1.3, fuse=False)
    assert "pm_mca_estep_mstats_defer_f64" in a and "pm_mca_estep_mstats_defer_f64" not in b
    assert "pm_mca_estep_f64" in b and "pm_mca_mstep_rows_f64" in b
    for k in ("W", "pi", "sigma", "Q"):
        np.testing.assert_allclose(na[k], nb[k], rtol=1e-9, atol=1e-12)


# ------------------------------------------------------------------------------------------------ (b) GSC
def _gsc_lds(H, Hp, gamma):
    """(bytes of the plain layout, bytes with the per-wavefront column accumulators) of gsc_estep_kernel
    (gsc_kernels.hip: gsc_shmem / gsc_shmem_lacc, ROWS = 16)."""
    from math import comb
    S = sum(comb(Hp, g) for g in range(2, min(gamma, Hp) + 1))
    plain = 8 * (8 * H + 16 * (48 + 4 * Hp * Hp) + (S + 3) // 4)
    return plain, plain + 8 * (12 * H + 1)


def _gsc_vs_oracle(D, H, Hp, gamma, N, seed, T=1.0, sigma_type="scalar"):
    from oracle import gsc_oracle as G
    from prosper_amd.em.camodels.gsc_et import GSC
    rng = np.random.RandomState(seed)
    gt = {"W": rng.normal(size=(D, H)), "pi": np.full(H, min(0.3, 2.0 / H)), "mu": np.full(H, 1.5), "psi_sq": np.eye(H),
          "sigma_sq": 1.0}
    y, _, _ = G.generate_gsc_data(gt, N, rng)
    Q = 0.05 * rng.normal(size=(H, H))
    params = {"W": gt["W"] + 0.1 * rng.normal(size=(D, H)), "pi": np.clip(gt["pi"] * rng.uniform(0.8, 1.3, size=H), 0.01, 0.9),
              "mu": gt["mu"] + 0.1 * rng.normal(size=H), "psi_sq": np.diag(rng.uniform(0.7, 1.4, size=H)) + Q @ Q.T,
              "sigma_sq": 1.2}
    if sigma_type == "diagonal":
        params["sigma_sq"] = rng.uniform(0.9, 1.5, size=D)
    elif sigma_type == "full":
        Qs = 0.1 * rng.normal(size=(D, D))
        params["sigma_sq"] = np.diag(rng.uniform(0.9, 1.5, size=D)) + Qs @ Qs.T
    model = G.make_model(D, H, Hp, gamma)
    m = GSC(D, H, Hp, gamma, sigma_type)
    assert np.array_equal(m.state_matrix, model["SM"])
    lpj, cand = m.compute_lpj(_An(T=1.0), _cp(params), {"y": y})
    cand = np.asarray(cand).astype(np.int64)
    assert np.array_equal(cand, G.select_hprimes(params, y, Hp))
    np.testing.assert_allclose(np.asarray(lpj), G.compute_lpj(model, params, y, cand), rtol=1e-9, atol=1e-8)   # (test_gsc_gpu.py's)
    ref, log = G.em_step(G.Anneal(T=T), model, _cp(params), y)
    m = GSC(D, H, Hp, gamma, sigma_type)
    names = _spy(m)
    new = m.step(_An(T=T), _cp(params), {"y": y})
    cond = np.linalg.cond(log["suff"]["xpt_szsz"].sum(0))
    tol = max(1e-8, 50 * cond * np.finfo(float).eps)
    for k in ("W", "pi", "mu", "psi_sq", "sigma_sq"):
        np.testing.assert_allclose(new[k], ref[k], rtol=10 * tol, atol=tol * max(1.0, np.abs(ref[k]).max()), err_msg=k)
    return names


# every V bucket of gsc_estep_kernel (H <= 16, 32, 64, 128, 256, 512) meets gamma = 5 .. 8 (G = 6 for 5, 6; G = 8 for 7, 8)
_GSC = [(H, Hp, g) for H, pairs in ((12, ((5, 5), (8, 8))), (24, ((6, 6), (7, 7))), (48, ((7, 5), (8, 8))),
                                    (100, ((8, 6), (7, 7))), (200, ((7, 5), (8, 8))), (400, ((6, 6), (8, 7))))
        for Hp, g in pairs]


@pytest.mark.parametrize("H,Hp,gamma", _GSC)
def test_gsc_gamma_above_4_matches_oracle(H, Hp, gamma):
    from prosper_amd import _lib
    plain, lacc = _gsc_lds(H, Hp, gamma)
    assert _lib.load().pm_gsc_supported(H, Hp, gamma) and plain <= 64 * 1024
    N = 160 if H <= 100 else 80
    names = _gsc_vs_oracle(24, H, Hp, gamma, N, H + 10 * Hp + gamma, T=1.1)
    assert "pm_gsc_estep_f64" in names, sorted(set(names))


def test_gsc_sweep_covers_both_lds_layouts():
    """The cases above run gsc_estep_kernel with the per-wavefront column accumulators in LDS (``lacc``, <= 53 KB) and
    without them."""
    lacc = [_gsc_lds(H, Hp, g)[1] <= 53 * 1024 for H, Hp, g in _GSC]
    assert any(lacc) and not all(lacc)


@pytest.mark.parametrize("sigma_type,Hp,gamma,H", [("scalar", 7, 4, 10), ("scalar", 7, 4, 40), ("diagonal", 7, 5, 20),
                                                   ("full", 7, 5, 20)])
def test_gsc_shipped_and_noise_models_match_oracle(sigma_type, Hp, gamma, H):
    names = _gsc_vs_oracle(25, H, Hp, gamma, 150, 7 * H + gamma, T=1.0 if sigma_type == "scalar" else 1.2,
                           sigma_type=sigma_type)
    assert "pm_gsc_estep_f64" in names, sorted(set(names))


# ------------------------------------------------------------------------------------------------ (b) DSC / TSC
def _xsc_problem(kind, D, H, N, seed, states=None):
    rng = np.random.RandomState(seed)
    if kind == "dsc":
        states = np.array(states)
        K = len(states)
        pi_gt = np.where(states == 0, 1 - 2.0 / H, (2.0 / H) / (K - 1))
        W_gt = rng.normal(size=(D, H)) * 2.0
        y = rng.choice(states, size=(N, H), p=pi_gt) @ W_gt.T + rng.normal(size=(N, D))
        pi0 = pi_gt * rng.uniform(0.8, 1.25, size=K)
        return y, {"W": W_gt + 0.2 * rng.normal(size=(D, H)), "pi": pi0 / pi0.sum(), "sigma": 1.1}
    pi_gt = 2.0 / H
    W_gt = rng.normal(size=(D, H)) * 2.0
    y = rng.choice([-1., 0., 1.], size=(N, H), p=[pi_gt / 2, 1 - pi_gt, pi_gt / 2]) @ W_gt.T + rng.normal(size=(N, D))
    return y, {"W": W_gt + 0.2 * rng.normal(size=(D, H)), "pi": pi_gt * 1.2, "sigma": 1.1}


def _xsc_vs_oracle(kind, D, H, Hp, gamma, N, seed, states=None, T=1.0, ncut=0.0, fuse=True):
    if kind == "dsc":
        from oracle import dsc_oracle as M
        from prosper_amd.em.camodels.dsc_et import DSC_ET
        mk = lambda: DSC_ET(D, H, Hp, gamma, states=np.array(states))
        model = M.make_model(D, H, Hp, gamma, np.array(states))
    else:
        from oracle import tsc_oracle as M
        from prosper_amd.em.camodels.tsc_et import TSC_ET
        mk = lambda: TSC_ET(D, H, Hp, gamma)
        model = M.make_model(D, H, Hp, gamma)
    y, params = _xsc_problem(kind, D, H, N, seed, states)
    an, dan = M.Anneal(T=T, Ncut_factor=ncut, anneal_prior=False), _An(T=T, Ncut_factor=ncut, anneal_prior=False)
    m = mk()
    data = m.select_Hprimes(_cp(params), {"y": y})
    cand = np.asarray(data["candidates"]).astype(np.int64)
    assert np.array_equal(cand, M.select_hprimes_vec(model, params["W"], params["pi"], params["sigma"], y))
    ss = m.E_step(dan, _cp(params), data)
    np.testing.assert_allclose(np.asarray(ss["logpj"]), M.e_step_vec(an, model, params["W"], params["pi"], params["sigma"], y, cand),
                               rtol=1e-10, atol=1e-9)
    ref, log = M.em_step(an, model, _cp(params), y, vec=True)
    m = mk()
    m.fuse_mstats = fuse
    names = _spy(m)
    new, hl = _logged(lambda: m.step(dan, _cp(params), {"y": y}))
    assert int(hl["N_use"][0]) == log["N_use"]
    np.testing.assert_allclose(float(hl["L"][0]), log["L"], rtol=1e-10)
    cond = np.linalg.cond(log["stats"]["Wq"])
    np.testing.assert_allclose(new["W"], ref["W"], rtol=0, atol=max(1e-8, 1e-13 * cond) * np.abs(ref["W"]).max())
    np.testing.assert_allclose(new["pi"], ref["pi"], rtol=1e-9)
    np.testing.assert_allclose(new["sigma"], ref["sigma"], rtol=1e-9)
    return m, names, new


@pytest.mark.parametrize("states,Hp,gamma,S", [([0., 1., 2.], 7, 5, 1596), ([0., 1., 2., 3.], 5, 5, 1008)])
@pytest.mark.parametrize("H", [40, 300])
def test_dsc_gamma5_matches_oracle_with_and_without_fused_statistics(states, Hp, gamma, S, H):
    """States with four or five non-zeros leave the energy table's fast path for the generic walk.  H <= 256: the 16-lane
    kernels; H > 256: none.  The E-step pass with the M-step statistics against the two passes."""
    from prosper_amd import _lib
    lib = _lib.load()
    out = {}
    for fuse in (True, False):
        N = 600 if H <= 256 else 2400
        m, names, new = _xsc_vs_oracle("dsc", 30, H, Hp, gamma, N, H + Hp + len(states), states=states, T=1.1, fuse=fuse)
        assert m.no_states == S
        assert bool(lib.pm_dsc_rows16_supported(H, Hp, S, len(states), 0)) == (H <= 256)
        can = bool(lib.pm_dsc_estep_mstats_supported(H, Hp, S, len(states), 0))
        assert ("pm_dsc_estep_mstats_f64" in names) == (fuse and can), sorted(set(names))
        assert ("pm_dsc_estep_f64" in names) == (not (fuse and can)), sorted(set(names))
        out[fuse] = new
    # the pass with the M-step statistics holds 1008 states (four values, (5, 5)) up to H = 256; the shipped set's 1596 take two
    # passes
    assert can == (S == 1008 and H <= 256)
    for k in ("W", "pi", "sigma"):
        np.testing.assert_allclose(out[True][k], out[False][k], rtol=1e-9, atol=1e-12)


def test_dsc_gamma5_truncation_step_matches_oracle():
    _, names, _ = _xsc_vs_oracle("dsc", 25, 10, 7, 5, 201, 5, states=[0., 1., 2.], T=1.4, ncut=0.6)
    assert "pm_dsc_estep_f64" in names and "pm_dsc_estep_mstats_f64" not in names


@pytest.mark.parametrize("H,N,ncut", [(40, 150, 0.0), (40, 150, 0.5), (256, 60, 0.0)])        # 2H = 512 at the end
def test_tsc_gamma5_matches_oracle(H, N, ncut):
    from oracle import tsc_oracle as M
    m, names, _ = _xsc_vs_oracle("tsc", 32, H, 7, 5, N, H + N, T=1.2, ncut=ncut)
    assert m.no_states == M.make_model(32, H, 7, 5)["no_states"] > 1000
    assert ("pm_dsc_estep_mstats_f64" in names) or ("pm_dsc_estep_f64" in names), sorted(set(names))
