"""BSC EM steps on incomplete data on the device, against the NumPy restatement tests/masked_train_reference.py
(pinned on the CPU by tests/test_masked_train_cpu.py): the reference's goldens at an all-ones mask, one case per branch of the
kernels, annealing, a shared mask against the project's own unmasked step, never-observed dimensions, whatever the holes
hold, bit for bit repeatable (runs, builds, step() against its three methods), an undisturbed unmasked loop, partial data,
the free energy, the refusals, the limits and two ranks.

Tolerances (the project's bounds for a step and for the masked path): W_new, pi, sigma to RTOL_STEP = 1e-8 (W relative to its
largest entry); L and the packed statistics to 1e-11 (each block relative to its largest entry).  Before comparing, every
test asserts on the reference that cond(A_d) < 1e6 for every observed dimension and that the selection gap exceeds 1e-9
relative in every row with an observed value."""
import functools

import numpy as np
import pytest

from conftest import golden
import masked_reference as MR
import masked_train_reference as T

pytestmark = pytest.mark.gpu

RTOL_STEP = 1e-8
RTOL_STAT = 1e-11
GAP = 1e-9
COND = 1e6


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def _bsc(D, H, Hp, g, **kw):
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    return BSC_ET(D, H, Hp, g, **kw)


def _same_bits(a, b, what=""):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, what
    assert np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64)), what


def _same_params(a, b, what=""):
    for k in ("W", "pi", "sigma", "mu"):
        _same_bits(a[k], b[k], "%s %s" % (what, k))


def _copy(p):
    return {k: np.array(v, copy=True) if isinstance(v, np.ndarray) else v for k, v in p.items()}


def _logged(fn, keys=("L", "N", "N_use", "W_kept")):
    """Run ``fn`` with the data log kept in memory: (result, {key: last value})."""
    from prosper_amd.utils.datalog import dlog, StoreInMemory
    h = dlog.set_handler(keys, StoreInMemory)
    try:
        out = fn()
    finally:
        dlog.remove_handler(h)
    return out, {k: v[-1].item() for k, v in h.tables.items() if k in keys}


def _rel(got, want):
    scale = float(np.abs(want).max()) if np.size(want) else 0.0
    return float(np.abs(np.asarray(got) - np.asarray(want)).max()) / (scale if scale > 0 else 1.0) if np.size(want) else 0.0


def _preconditions(tag, params, Y, M, Hp, ref_log):
    sc = MR.score_bsc(np.where(M, Y, 0.0), M, np.asarray(params["W"]), params.get("mu"))
    gap = MR.boundary_gap(sc, Hp, True)[np.asarray(M).any(axis=1)]
    cond = T.conditioning(ref_log, M)
    print("%-28s reference: largest cond(A_d) %.2e (needs < %.0e), smallest selection gap %.2e (needs > %.0e)"
          % (tag, cond, COND, gap.min(), GAP))
    assert cond < COND, cond
    assert (gap > GAP).all(), gap.min()


def _packed(m, D, H):
    """The packed statistics of the model's last masked M-step: A (D, H, H), r (H, D), sum E[s] (H), 4 scalars."""
    t = m._ws["mt_packed"].cpu().numpy()
    nA = D * H * H
    return t[:nA].reshape(D, H, H), t[nA:nA + H * D].reshape(H, D), t[nA + H * D:nA + H * D + H], t[nA + H * D + H:]


def _check_step(tag, m, new, logd, ref, rlog, D, H, stats=True):
    W = np.asarray(new["W"])
    errs = {"W": _rel(W, ref["W"]), "pi": abs(new["pi"] / ref["pi"] - 1), "sigma": abs(new["sigma"] / ref["sigma"] - 1),
            "L": abs(logd["L"] / rlog["L"] - 1)}
    if stats:
        A, r, sumE, sc = _packed(m, D, H)
        tot = rlog["tot"]
        errs.update(A=_rel(A, tot["A"]), r=_rel(r, tot["r"]), sumE=_rel(sumE, tot["sumE"]),
                    energy=abs(sc[0] / tot["sum_energy"] - 1), lse=abs(sc[1] / tot["sum_lse"] - 1))
        assert sc[2] == tot["N"] and sc[3] == tot["sum_dn"], sc
    print("%-28s " % tag + " ".join("%s %.2e" % kv for kv in errs.items()))
    assert W.shape == (D, H) and W.dtype == np.float64
    for k in ("W", "pi", "sigma"):
        assert errs[k] <= RTOL_STEP, (tag, k, errs[k])
    for k in set(errs) - {"W", "pi", "sigma"}:
        assert errs[k] <= RTOL_STAT, (tag, k, errs[k])
    assert logd["N"] == rlog["N"] and logd["N_use"] == rlog["N"]
    assert logd["W_kept"] == rlog["W_kept"] == m.W_kept
    kept = np.nonzero(rlog["kept"])[0]
    return kept


# ------------------------------------------------------------------------------------------------ 1: the reference's goldens
@pytest.mark.parametrize("case", ["bsc_step_c1_plain", "bsc_step_h32"])
def test_all_ones_mask_against_the_reference_goldens(dev, case):
    g = golden(case + ".npz")
    D, H, Hp, gm = int(g["D"]), int(g["H"]), int(g["Hprime"]), int(g["gamma"])
    an = T.Anneal(T=float(g["T"]), anneal_prior=bool(g["anneal_prior"]))
    params = {"W": g["W"].copy(), "pi": float(g["pi"]), "sigma": float(g["sigma"])}
    m = _bsc(D, H, Hp, gm)
    data = {"y": g["y"], "mask": np.ones(g["y"].shape, dtype=bool)}
    new, logd = _logged(lambda: m.step(an, params, data))
    scale = np.abs(g["W_new"]).max()
    print("%s: W %.2e pi %.2e sigma %.2e L %.2e" % (case, np.abs(new["W"] - g["W_new"]).max() / scale,
                                                  abs(new["pi"] / g["pi_new"] - 1), abs(new["sigma"] / g["sigma_new"] - 1),
                                                  abs(logd["L"] / g["L"] - 1)))
    np.testing.assert_allclose(new["W"], g["W_new"], rtol=RTOL_STEP, atol=RTOL_STEP * scale)
    np.testing.assert_allclose(new["pi"], g["pi_new"], rtol=RTOL_STEP)
    np.testing.assert_allclose(new["sigma"], g["sigma_new"], rtol=RTOL_STEP)
    np.testing.assert_allclose(logd["L"], g["L"], rtol=RTOL_STAT)
    assert logd["N"] == int(g["N"]) and logd["W_kept"] == 0


# ------------------------------------------------------------------------------------------------------- 2: branch cases
# (D, H, H', gamma, N, seed): 50 % observed, row 0 fully observed, row 1 unobserved, the last dimension never observed.
# Which branch a shape takes is named in DESIGN 4.17 (the pair kernel's tile is 64 dimensions x HB = min(H, 256 // H) latent
# rows x H columns):
BRANCH = [(20, 6, 6, 6, 37, 0),        # every state; one tile (HB = H)
          (70, 24, 6, 3, 130, 0),      # two dimension slabs, the second ragged (6); HB = 10: blocks 10, 10, 4 (ragged)
          (33, 65, 6, 3, 400, 1),      # HB = 3: 22 blocks, the last ragged (2); latents beyond the first 64
          (24, 130, 12, 3, 900, 0),    # 66 pairs: a lane of the rows kernel owns two; HB = 1; S = 286: two state chunks
          (8, 256, 16, 2, 3000, 0),    # H and H' at their limits: 120 pairs, 128 KB tile rows
          (1024, 10, 5, 3, 64, 0),     # widest D: 16 slabs, the last full
          (16, 8, 5, 3, 8269, 0),      # second trip of the rows kernels' grid-stride loops (2048 workgroups of 4 rows)
          (64, 4, 3, 2, 40, 0),        # exactly one full slab
          (65, 16, 4, 2, 200, 0),      # a ragged slab of one dimension; HB = H = 16
          (10, 3, 1, 1, 20, 1)]        # H' = 1: no pairs and no table states, diagonal systems


@functools.lru_cache(maxsize=None)
def _branch_problem(D, H, Hp, g, N, seed, T_=1.0, prior=False):
    rng = np.random.RandomState(1000 * seed + D + H + N)
    params, Y, M = T.model_problem(rng, D, H, N)
    an = T.Anneal(T=T_, anneal_prior=prior)
    Yh = np.where(M, Y, np.nan)
    ref, rlog = T.step(an, params, Yh, M, Hp, g)
    return params, Y, M, Yh, an, ref, rlog


@pytest.mark.parametrize("D,H,Hp,g,N,seed", BRANCH)
def test_branch_cases(dev, D, H, Hp, g, N, seed):
    params, Y, M, Yh, an, ref, rlog = _branch_problem(D, H, Hp, g, N, seed)
    tag = "%d-%d-%d-%d-%d" % (D, H, Hp, g, N)
    _preconditions(tag, params, Y, M, Hp, rlog)
    m = _bsc(D, H, Hp, g)
    calls = []
    orig = m._call
    m._call = lambda label, entry, *a: (calls.append(entry), orig(label, entry, *a))[1]
    p_in = _copy(params)
    new, logd = _logged(lambda: m.step(an, params, {"y": Yh, "mask": M}))
    assert {"pm_masked_prepare_f64", "pm_bsc_masked_estep_f64", "pm_rows_lse_f64", "pm_bsc_mtrain_rows_f64",
            "pm_col_sum_ordered_f64", "pm_bsc_mtrain_pairs_f64", "pm_spd_inverse_batch_f64",
            "pm_bsc_mtrain_solve_f64"} <= set(calls), calls
    np.testing.assert_array_equal(params["W"], p_in["W"])
    kept = _check_step(tag, m, new, logd, ref, rlog, D, H)
    # the never-observed dimension keeps its row of W bit for bit and is the one counted
    assert list(kept) == [D - 1] and logd["W_kept"] == 1
    _same_bits(np.asarray(new["W"])[D - 1], params["W"][D - 1], "kept row")
    if N > 8192:
        # per-row statistics: the tail rows (second trip of the grid-stride loop) against NumPy, and everything bit for bit
        # against 4096-row shards
        import torch
        full = {k: m._ws[k].clone() for k in ("mt_es", "mt_q2", "mt_energy", "mt_lse")}
        for k, want in (("mt_es", rlog["Es"]), ("mt_q2", rlog["q2"]), ("mt_energy", rlog["energy"]), ("mt_lse", rlog["lse"])):
            got = full[k].cpu().numpy()
            assert _rel(got[8192:], want[8192:]) <= RTOL_STAT, k
        for r0 in range(0, N, 4096):
            sl = slice(r0, min(N, r0 + 4096))
            m.step(an, _copy(params), {"y": Yh[sl], "mask": M[sl]})
            for k in full:
                assert torch.equal(m._ws[k], full[k][sl]), (k, r0)


# --------------------------------------------------------------------------------------------------------- 3: annealing
@pytest.mark.parametrize("prior", [True, False])
def test_annealed_step(dev, prior):
    D, H, Hp, g, N, seed = BRANCH[1]
    params, Y, M, Yh, an, ref, rlog = _branch_problem(D, H, Hp, g, N, seed, 1.7, prior)
    _preconditions("T=1.7 prior=%s" % prior, params, Y, M, Hp, rlog)
    m = _bsc(D, H, Hp, g)
    new, logd = _logged(lambda: m.step(an, _copy(params), {"y": Yh, "mask": M}))
    _check_step("T=1.7 anneal_prior=%s" % prior, m, new, logd, ref, rlog, D, H)


# ------------------------------------------------------------------------------------------------------- 4: shared mask
def test_shared_mask_equals_the_unmasked_step_on_the_sub_model(dev):
    rng = np.random.RandomState(5)
    D, H, Hp, g, N = 40, 12, 5, 3, 300
    params, Y, _ = T.model_problem(rng, D, H, N, never=False)
    obs = np.sort(rng.permutation(D)[:24])
    M = np.zeros((N, D), dtype=bool)
    M[:, obs] = True
    an = T.Anneal(T=1.3, anneal_prior=True)
    _, rlog = T.step(an, params, np.where(M, Y, 0.0), M, Hp, g)
    _preconditions("shared mask", params, Y, M, Hp, rlog)
    new, logd = _logged(lambda: _bsc(D, H, Hp, g).step(an, _copy(params), {"y": np.where(M, Y, np.nan), "mask": M}))
    sub = {"W": params["W"][obs].copy(), "pi": params["pi"], "sigma": params["sigma"]}
    ref, rlogd = _logged(lambda: _bsc(len(obs), H, Hp, g).step(an, sub, {"y": np.ascontiguousarray(Y[:, obs])}),
                         keys=("L", "N"))
    W = np.asarray(new["W"])
    scale = np.abs(ref["W"]).max()
    print("shared mask: W %.2e pi %.2e sigma %.2e L %.2e" % (np.abs(W[obs] - ref["W"]).max() / scale,
                                                             abs(new["pi"] / ref["pi"] - 1),
                                                             abs(new["sigma"] / ref["sigma"] - 1),
                                                             abs(logd["L"] / rlogd["L"] - 1)))
    np.testing.assert_allclose(W[obs], ref["W"], rtol=RTOL_STEP, atol=RTOL_STEP * scale)
    np.testing.assert_allclose([new["pi"], new["sigma"]], [ref["pi"], ref["sigma"]], rtol=RTOL_STEP)
    np.testing.assert_allclose(logd["L"], rlogd["L"], rtol=RTOL_STAT)
    rest = np.setdiff1d(np.arange(D), obs)
    _same_bits(W[rest], params["W"][rest], "rows of W nobody observed")
    assert logd["W_kept"] == len(rest)


# ------------------------------------------------------------------------------------------- 5: never-observed dimensions
def test_never_observed_dimensions_keep_their_rows(dev):
    D, H, Hp, g, N, seed = BRANCH[1]
    params, Y, M, Yh, an, _, _ = _branch_problem(D, H, Hp, g, N, seed)
    M = M.copy()
    never = [3, 64, D - 1]                       # (one in each slab, and the last)
    M[:, never] = False
    Yh = np.where(M, Y, np.nan)
    ref, rlog = T.step(an, params, Yh, M, Hp, g)
    _preconditions("never observed", params, Y, M, Hp, rlog)
    m = _bsc(D, H, Hp, g)
    new, logd = _logged(lambda: m.step(an, _copy(params), {"y": Yh, "mask": M}))
    kept = _check_step("never observed", m, new, logd, ref, rlog, D, H)
    assert list(kept) == never and logd["W_kept"] == len(never) == m.W_kept
    _same_bits(np.asarray(new["W"])[never], params["W"][never], "kept rows")


# ---------------------------------------------------------------------------------------------------- 6: what holes hold
def test_unobserved_entries_change_no_bit(dev):
    D, H, Hp, g, N, seed = BRANCH[1]
    params, Y, M, _, an, _, _ = _branch_problem(D, H, Hp, g, N, seed)
    outs = []
    for fill in (0.0, np.nan, np.inf, 1e300):
        m = _bsc(D, H, Hp, g)
        new, logd = _logged(lambda: m.step(an, _copy(params), {"y": np.where(M, Y, fill), "mask": M}))
        assert np.isfinite(new["W"]).all() and np.isfinite([new["pi"], new["sigma"], logd["L"]]).all()
        outs.append((new, logd["L"]))
    for new, L in outs[1:]:
        _same_params(new, outs[0][0], "fill")
        assert L == outs[0][1]


# ---------------------------------------------------------------------------------------------------------- 7: same bits
def test_same_bits_runs_builds_and_entry_points(dev):
    D, H, Hp, g, N, seed = BRANCH[2]
    params, Y, M, Yh, an, _, _ = _branch_problem(D, H, Hp, g, N, seed)
    data = lambda: {"y": Yh, "mask": M}
    m = _bsc(D, H, Hp, g)
    first, l1 = _logged(lambda: m.step(an, _copy(params), data()))
    second, l2 = _logged(lambda: m.step(an, _copy(params), data()))
    _same_params(first, second, "second run")
    assert l1 == l2
    fresh = _bsc(D, H, Hp, g).step(an, _copy(params), data())
    _same_params(first, fresh, "fresh model")
    md = _bsc(D, H, Hp, g)
    md.deterministic = True
    det, l3 = _logged(lambda: md.step(an, _copy(params), data()))
    _same_params(first, det, "deterministic library")
    assert l1 == l3
    # the three methods called from outside, one after the other
    mo = _bsc(D, H, Hp, g)
    p = _copy(params)
    d = mo.select_Hprimes(p, data())
    ss = mo.E_step(an, p, d)
    out, l4 = _logged(lambda: mo.M_step(an, p, ss, d))
    _same_params(first, out, "select_Hprimes / E_step / M_step")
    assert l1 == l4
    # ... and with the candidates and log-joints taken to the host in between
    mo = _bsc(D, H, Hp, g)
    p = _copy(params)
    d = mo.select_Hprimes(p, data())
    cand = np.asarray(d["candidates"])
    ss = mo.E_step(an, p, d)
    out = mo.M_step(an, p, {"logpj": np.asarray(ss["logpj"])}, {"y": Yh, "mask": M, "candidates": cand})
    _same_params(first, out, "host candidates and log-joints")


# ------------------------------------------------------------------------------------------------------ 8: order of calls
def test_masked_step_leaves_the_unmasked_loop_alone(dev):
    """(On the deterministic library: the default build's unmasked M-step adds with atomics, so two identical unmasked steps
    differ in their last bits by themselves -- only there can "the same bits" be asked of the unmasked loop at all.)"""
    D, H, Hp, g, N, seed = BRANCH[1]
    params, Y, M, Yh, an, _, _ = _branch_problem(D, H, Hp, g, N, seed)

    def model():
        m = _bsc(D, H, Hp, g)
        m.deterministic = True
        return m
    alone = model()
    a1 = alone.step(an, _copy(params), {"y": Y})
    a2 = alone.step(an, _copy(a1), {"y": Y})
    mixed = model()
    b1 = mixed.step(an, _copy(params), {"y": Y})
    mixed.step(an, _copy(params), {"y": Yh, "mask": M})
    b2 = mixed.step(an, _copy(b1), {"y": Y})
    _same_params(a1, b1, "first unmasked step")
    _same_params(a2, b2, "unmasked step behind a masked one")
    first = model()
    first.step(an, _copy(params), {"y": Yh, "mask": M})
    _same_params(a1, first.step(an, _copy(params), {"y": Y}), "unmasked step of a model that began masked")


# -------------------------------------------------------------------------------------------------------- 9: partial data
def test_partial_data_takes_the_masks_rows_along(dev):
    D, H, Hp, g, N, seed = BRANCH[1]
    params, Y, M, Yh, _, _, _ = _branch_problem(D, H, Hp, g, N, seed)
    an = T.Anneal(T=1.0, partial=0.5)
    np.random.seed(77)
    got, lg = _logged(lambda: _bsc(D, H, Hp, g).step(an, _copy(params), {"y": Yh, "mask": M}))
    np.random.seed(77)
    sel = np.sort(np.random.permutation(N)[:int(np.ceil(N * 0.5))])
    want, lw = _logged(lambda: _bsc(D, H, Hp, g).step(T.Anneal(T=1.0), _copy(params), {"y": Yh[sel], "mask": M[sel]}))
    _same_params(got, want, "partial")
    assert lg == lw and lg["N"] == len(sel)
    ref, rlog = T.step(T.Anneal(T=1.0), params, Yh[sel], M[sel], Hp, g)
    assert _rel(got["W"], ref["W"]) <= RTOL_STEP and rlog["W_kept"] == lg["W_kept"]


# ------------------------------------------------------------------------------------------------------- 10: free energy
def test_free_energy_is_the_masked_log_likelihood(dev):
    D, H, Hp, g, N, seed = BRANCH[1]
    params, Y, M, Yh, an, _, rlog = _branch_problem(D, H, Hp, g, N, seed)
    m = _bsc(D, H, Hp, g)
    _, logd = _logged(lambda: m.step(an, _copy(params), {"y": Yh, "mask": M}))
    ll = m.log_likelihood(_copy(params), {"y": Yh, "mask": M})
    A_pg = T.pi_gamma_factors(params["pi"], H, g)[0]
    want = ll / N - np.log(A_pg)
    print("L %.12f, log_likelihood / N - log A %.12f (relative %.2e)" % (logd["L"], want, abs(logd["L"] / want - 1)))
    np.testing.assert_allclose(logd["L"], want, rtol=RTOL_STAT)


def test_exact_em_is_monotone_and_follows_numpy(dev):
    Ls_ref, p_ref = T.exact_em_trajectory()
    params, Yh, M = T.exact_em_start()
    D, H = params["W"].shape
    m = _bsc(D, H, H, H)
    an = T.Anneal(T=1.0)
    Ls = []
    for _ in range(25):
        params, logd = _logged(lambda: m.step(an, params, {"y": Yh, "mask": M}))
        Ls.append(logd["L"])
    Ls = np.array(Ls)
    drift = {"W": _rel(params["W"], p_ref["W"]), "pi": abs(params["pi"] / p_ref["pi"] - 1),
             "sigma": abs(params["sigma"] / p_ref["sigma"] - 1), "L": float(np.abs(Ls / np.array(Ls_ref) - 1).max())}
    print("exact EM, 25 steps: smallest step of L %.3e; drift against NumPy %s" % (np.diff(Ls).min(), drift))
    assert (Ls[1:] >= Ls[:-1] - 1e-10 * np.abs(Ls[:-1])).all(), np.diff(Ls).min()
    assert max(drift.values()) <= 1e-6, drift


# ----------------------------------------------------------------------------------------------------------- 11: refusals
def _no_launch(m):
    calls = []
    orig = m._call
    m._call = lambda label, entry, *a: (calls.append(entry), orig(label, entry, *a))[1]
    return calls


def _others(D, H):
    from prosper_amd.em.camodels.dsc_et import DSC_ET
    from prosper_amd.em.camodels.tsc_et import TSC_ET
    from prosper_amd.em.camodels.gsc_et import GSC
    from prosper_amd.em.camodels.mca_et import MCA_ET
    from prosper_amd.em.camodels.mmca_et import MMCA_ET
    from prosper_amd.em.mixturemodels.MoG import MoG
    from prosper_amd.em.mixturemodels.MoP import MoP
    return [DSC_ET(D, H, 3, 2, states=np.array([0., 1., 2.])), TSC_ET(D, H, 3, 2), GSC(D, H, 3, 2), MCA_ET(D, H, 3, 2),
            MMCA_ET(D, H, 3, 2), MoG(D, H, sigmas_sq_type="diagonal"), MoP(D, H)]


def test_other_models_refuse_a_mask_by_name(dev):
    D, H, N = 8, 4, 10
    rng = np.random.RandomState(0)
    data = {"y": np.abs(rng.normal(size=(N, D))), "mask": np.ones((N, D), dtype=bool)}
    an = T.Anneal(T=1.0)
    for m in _others(D, H):
        calls = _no_launch(m) if hasattr(m, "_call") else []
        for fn in (lambda: m.step(an, {}, data), lambda: m.E_step(an, {}, data), lambda: m.M_step(an, {}, {}, data)):
            with pytest.raises(NotImplementedError, match="mask"):
                fn()
        assert calls == [], (type(m).__name__, calls)


def test_bsc_refusals_before_any_launch(dev):
    D, H, Hp, g, N = 12, 6, 4, 2, 20
    rng = np.random.RandomState(1)
    params, Y, M = T.model_problem(rng, D, H, N)
    data = {"y": Y, "mask": M}

    def refused(m, exc, an=T.Anneal(T=1.0), d=data):
        calls = _no_launch(m)
        for fn in (lambda: m.step(an, _copy(params), dict(d)), lambda: m.E_step(an, _copy(params), dict(d)),
                   lambda: m.M_step(an, _copy(params), {"logpj": np.zeros((N, 1))}, dict(d))):
            with pytest.raises(exc):
                fn()
        assert calls == [], calls

    refused(_bsc(D, H, Hp, g, to_learn=["W", "pi", "sigma", "mu"]), NotImplementedError)
    refused(_bsc(D, H, Hp, g), NotImplementedError, an=T.Anneal(T=1.0, Ncut_factor=0.5))
    refused(_bsc(D, H, Hp, g), ValueError, d={"y": Y, "mask": M[:, :-1]})
    refused(_bsc(D, H, Hp, g), ValueError, d={"y": Y, "mask": M[:-1]})
    m = _bsc(D, H, Hp, g)
    calls = _no_launch(m)
    with pytest.raises(ValueError):
        m.select_Hprimes(_copy(params), {"y": Y, "mask": M[:, :-1]})
    assert calls == []


def test_one_past_each_limit(dev):
    from prosper_amd import _lib
    an = T.Anneal(T=1.0)
    for D, H, Hp, N in ((4, 257, 4, 6), (4, 20, 17, 6), ((1 << 28) // (64 * 64) + 1, 64, 4, 1)):
        m = _bsc(D, H, Hp, 2)
        calls = _no_launch(m)

        class Shape(object):       # (the limits are checked from the shapes alone: nothing of D H^2 is allocated)
            shape = (N, D)
        with pytest.raises(_lib.HipError):
            m.step(an, {"W": None, "pi": 0.1, "sigma": 1.0}, {"y": Shape(), "mask": Shape()})
        assert calls == [] and not hasattr(m, "W_kept")


def test_to_learn_subsets(dev):
    D, H, Hp, g, N, seed = BRANCH[1]
    params, Y, M, Yh, an, ref, rlog = _branch_problem(D, H, Hp, g, N, seed)
    m = _bsc(D, H, Hp, g, to_learn=["pi"])
    calls = _no_launch(m)
    new = m.step(an, _copy(params), {"y": Yh, "mask": M})
    _same_bits(new["W"], params["W"])
    assert new["sigma"] == params["sigma"] and "pm_bsc_mtrain_pairs_f64" not in calls
    np.testing.assert_allclose(new["pi"], ref["pi"], rtol=RTOL_STEP)
    m = _bsc(D, H, Hp, g, to_learn=["W", "sigma"])
    new = m.step(an, _copy(params), {"y": Yh, "mask": M})
    assert new["pi"] == params["pi"] and _rel(new["W"], ref["W"]) <= RTOL_STEP
    np.testing.assert_allclose(new["sigma"], ref["sigma"], rtol=RTOL_STEP)


# ---------------------------------------------------------------------------------------------------------- 12: two ranks
def test_two_ranks_over_gloo(dev):
    """tests/masked_train_world2_gpu_worker.py: two processes, a world_size-2 gloo group on the one GPU; after 3 masked EM
    steps both ranks hold bitwise identical parameters, within tolerance of the one-rank run on the concatenated shards."""
    import os
    import socket
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    worker = os.path.join(here, "masked_train_world2_gpu_worker.py")
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    procs = []
    for rank in range(2):
        e = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                 RANK=str(rank), WORLD_SIZE="2")
        procs.append(subprocess.Popen([sys.executable, worker], env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                      text=True))
    outs = []
    try:
        for pr in procs:
            outs.append(pr.communicate(timeout=300))
    finally:
        for pr in procs:
            if pr.poll() is None:
                pr.kill()
    for rank, (pr, (out, err)) in enumerate(zip(procs, outs)):
        assert pr.returncode == 0 and ("ok %d" % rank) in out.split("\n"), "rank %d\n%s\n%s" % (rank, out[-2000:], err[-4000:])
