"""inference(..., exact=True) of BSC, MCA and MMCA on the device, at D = 16, H in {3, 6, 12}, N = 40: against the
NumPy enumeration of every state, against encode(exact=True) and log_likelihood(exact=True), against the project's own
truncated call at H' = gamma = H, bit for bit across calls, builds, row orders and shards, with a training run undisturbed,
and every refusal before any launch.

Tolerances: 1e-11 relative to the row's largest compared magnitude, floor 1 (RTOL of tests/test_exact_kernels_gpu.py); 2e-11
against the truncated path, each side being within 1e-11 of the truth (tests/test_reconstruct_exact_gpu.py).  States are
compared for equality: the reference (tests/infer_exact_reference.py) asserts for every row that consecutive entries among
the topK + 1 best differ by more than 1e-9 max(1, |l|) in its own longdouble values, so rounding cannot swap neighbours.
"""
import functools

import numpy as np
import pytest

import exact_kernels_reference as R
import infer_exact_reference as IR
from test_reconstruct_gpu import _problem

pytestmark = pytest.mark.gpu

RTOL = 1e-11
D, N = 16, 40
MODELS = ("bsc", "mca", "mmca")
HS = (3, 6, 12)


class _An(dict):
    crit_params = []

    def __missing__(self, k):
        return 0.0

    def as_dict(self):
        return dict(self)


T1 = _An(T=1.0)


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _case(name, H, Hp=3, g=2):
    """(model, params, Y, l): the problem and the reference's (N, 2^H) longdouble log-joints from the model's own
    ``_loglik_exact`` operands, computed once and shared."""
    m, p, Y, _, _ = _problem(name, np.random.RandomState(100 + H), D, H, N, min(Hp, H), min(g, H))
    kind, a, sc = m._loglik_exact({k: np.array(v, copy=True) for k, v in p.items()})
    if kind == "lin":
        l = IR.lin_table(Y, a.get("mu"), a["P"], a["G"], a["logp"], a["values"])
    else:
        l = IR.mca_table(Y, a["Wrho"], sc["inv_rho"], sc["signed"], sc["lp1"], sc["lp0"], sc["inv_s2"])
    l.setflags(write=False)
    return m, p, Y, l


def _entries(m):
    calls = []
    orig = m._call
    m._call = lambda label, entry, *args: (calls.append(entry), orig(label, entry, *args))[1]
    return calls


def _bits(a, b, what):
    for k in ("s", "p", "m", "gamma", "Hprime"):
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k)
        assert x.tobytes() == y.tobytes(), (what, k)


def _states_of(idx, H):
    return ((idx[:, :, None] >> np.arange(H)[None, None, :]) & 1).astype(np.int8)


def _rel(got, want, fin=None):
    want = np.asarray(want, dtype=np.float64)
    fin = np.isfinite(want) if fin is None else fin
    assert np.array_equal(got[~fin], want[~fin])
    scale = np.maximum(1.0, np.max(np.where(fin, np.abs(want), 0.0), axis=-1, keepdims=True))
    return float(np.max(np.where(fin, np.abs(np.where(fin, got, 0.0) - np.where(fin, want, 0.0)), 0.0) / scale, initial=0.0))


# ------------------------------------------------------------------------------------------ 1: against NumPy enumeration
@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("name", MODELS)
def test_against_numpy(dev, name, H):
    m, p, Y, l = _case(name, H)
    topK = 10
    IR.assert_margin(l, topK)                                   # every row
    ridx, rl, rv = IR.topk_rows(l, topK)
    cols = ridx.shape[1]
    q = R.lse_rows(l)[1]
    bits = _states_of(np.arange(1 << H)[None, :], H)[0].astype(IR.LD)
    marg = np.asarray(q @ bits, dtype=np.float64)
    p_in = {k: np.array(v, copy=True) for k, v in p.items()}
    calls = _entries(m)
    try:
        lin = m.inference(T1, p, {"y": Y}, topK=topK, exact=True)
        log = m.inference(T1, p, {"y": Y}, topK=topK, logprob=True, exact=True)
    finally:
        del m._call
    for k in p_in:
        np.testing.assert_array_equal(p[k], p_in[k])
    assert "pm_infer_exact_%s_f64" % ("lin" if name == "bsc" else "mca") in calls
    assert not [c for c in calls if "estep" in c or "select" in c or "topk" in c], calls
    for res in (lin, log):
        assert res["s"].shape == (N, topK, H) and res["s"].dtype == np.int8 and res["p"].shape == (N, topK)
        assert np.array_equal(res["s"][:, :cols], _states_of(ridx, H)) and not res["s"][:, cols:].any()
        assert not res["p"][:, cols:].any()
        assert np.array_equal(res["gamma"], np.full(N, float(H))) and np.array_equal(res["Hprime"], np.full(N, float(H)))
    e1 = _rel(log["p"][:, :cols], rl - rv[:, None])
    e2 = _rel(lin["p"][:, :cols], np.exp(rl - rl[:, :1]))
    e3 = _rel(lin["m"], marg)
    with np.errstate(divide="ignore"):
        e4 = _rel(log["m"], np.log(marg))
    print("inference exact %s H=%d: log p %.3e  p %.3e  m %.3e  log m %.3e (bound %.0e)" % (name, H, e1, e2, e3, e4, RTOL))
    assert np.all(lin["p"][:, 0] == 1.0)
    assert max(e1, e2, e3, e4) <= RTOL


# -------------------------------------------------------------------------------------------------- 2: against encode
@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("name", MODELS)
def test_marginals_are_encodes_bits(dev, name, H):
    m, p, Y, _ = _case(name, H)
    res = m.inference(T1, p, {"y": Y}, topK=2, exact=True)
    prob = m.encode(p, {"y": Y}, exact=True)[1]
    assert res["m"].dtype == prob.dtype and res["m"].tobytes() == prob.tobytes()


# ------------------------------------------------------------------------------------------ 3: against log_likelihood
@pytest.mark.parametrize("name", MODELS)
def test_the_whole_space_sums_to_one_and_to_the_likelihood(dev, name):
    H = 3
    m, p, Y, l = _case(name, H)
    res = m.inference(T1, p, {"y": Y}, topK=IR.MAX_TOPK, logprob=True, exact=True)
    assert not res["s"][:, 8:].any() and not res["p"][:, 8:].any()
    codes = (res["s"][:, :8].astype(np.int64) << np.arange(H)).sum(axis=-1)
    assert np.array_equal(np.sort(codes, axis=1), np.tile(np.arange(8), (N, 1)))
    assert np.max(np.abs(np.exp(res["p"][:, :8]).sum(axis=1) - 1.0)) <= RTOL
    # v_n + row constant = log_likelihood(exact=True) per datapoint: v_n = l_n(s) - p_n(s) for any listed state
    rows = m.log_likelihood(p, {"y": Y}, per_datapoint=True, exact=True)
    kind, a, sc = m._loglik_exact({k: np.array(v, copy=True) for k, v in p.items()})
    rl = np.asarray(IR.topk_rows(l, 1)[1][:, 0], dtype=np.float64)
    v = rl - res["p"][:, 0]
    if kind == "lin":
        X = Y - (0.0 if a.get("mu") is None else a["mu"][None, :])
        const = sc["cst"] + sc["qcoef"] * (X * X).sum(axis=1)
    else:
        const = sc["cst"] - 0.5 * sc["inv_s2"] * (Y * Y).sum(axis=1)
    assert np.max(np.abs(v + const - rows) / np.maximum(1.0, np.abs(rows))) <= RTOL


# ------------------------------------------------------------------------------------------ 4: against the truncated call
@pytest.mark.parametrize("name", MODELS)
def test_against_the_truncated_call_at_full_width(dev, name):
    H, topK = 6, 10
    small, p, Y, l = _case(name, H)
    full = _problem(name, np.random.RandomState(0), D, H, 1, H, H)[0]
    IR.assert_margin(l, topK)
    scale = np.maximum(1.0, np.abs(np.asarray(IR.topk_rows(l, topK + 1)[1], dtype=np.float64)))
    for logprob in (False, True):
        got = small.inference(T1, p, {"y": Y}, topK=topK, logprob=logprob, exact=True)
        want = full.inference(T1, {k: np.array(v, copy=True) for k, v in p.items()}, {"y": Y}, topK=topK, logprob=logprob,
                              adaptive=False)
        assert np.array_equal(got["s"], want["s"]), name                        # every row
        err = _rel(got["p"], want["p"])
        print("inference exact %s against H'=gamma=H, logprob=%s: %.3e (bound 2e-11)" % (name, logprob, err))
        assert err <= 2e-11
    # the margin on the truncated scores themselves: consecutive gaps among its topK + 1 best
    tr = full.inference(T1, {k: np.array(v, copy=True) for k, v in p.items()}, {"y": Y}, topK=topK + 1, logprob=True,
                        adaptive=False)["p"]
    assert np.all(tr[:, :-1] - tr[:, 1:] > IR.MARGIN * np.maximum(scale[:, :-1], scale[:, 1:]))


# ------------------------------------------------------------------------------------------ 5: bits and the training state
@pytest.mark.parametrize("name,H", [("bsc", 12), ("mca", 6), ("mmca", 12)])
def test_bits_across_calls_builds_row_order_and_shards(dev, name, H):
    m, p, Y, _ = _case(name, H)
    for logprob in (False, True):
        a = m.inference(T1, p, {"y": Y}, logprob=logprob, exact=True)
        _bits(m.inference(T1, p, {"y": Y}, logprob=logprob, exact=True), a, "second call")
        m.deterministic = True
        try:
            _bits(m.inference(T1, p, {"y": Y}, logprob=logprob, exact=True), a, "the deterministic library")
        finally:
            m.deterministic = False
        perm = np.random.RandomState(2).permutation(N)
        _bits(m.inference(T1, p, {"y": Y[perm]}, logprob=logprob, exact=True), {k: v[perm] for k, v in a.items()}, "permutation")
        _bits(m.inference(T1, p, {"y": Y[10:30]}, logprob=logprob, exact=True), {k: v[10:30] for k, v in a.items()}, "shard")
    _bits(m.inference(T1, p, {"y": Y}, adaptive=False, exact=True), m.inference(T1, p, {"y": Y}, exact=True), "adaptive")
    empty = m.inference(T1, p, {"y": np.zeros((0, D))}, topK=4, exact=True)
    assert empty["s"].shape == (0, 4, H) and empty["p"].shape == (0, 4) and empty["m"].shape == (0, H)


def test_a_nan_row_raises(dev):
    from prosper_amd import _lib
    m, p, Y, _ = _case("bsc", 6)
    Y = Y.copy()
    Y[7, 1] = np.nan
    with pytest.raises(_lib.HipError, match="NaN"):
        m.inference(T1, p, {"y": Y}, exact=True)


def test_training_undisturbed(dev):
    from prosper_amd.em.annealing import LinearAnnealing
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    rng = np.random.RandomState(14)
    Dt, H, Nt = 16, 8, 600
    p0 = {"W": rng.normal(size=(Dt, H)), "pi": 2.0 / H, "sigma": 1.2}
    Y = (rng.uniform(size=(Nt + 40, H)) < 2.0 / H) @ p0["W"].T + rng.normal(size=(Nt + 40, Dt))

    def train(interleave):
        m = BSC_ET(Dt, H, 5, 3)
        m.deterministic = True
        a = LinearAnnealing(4)
        a["T"] = [(0, 2.), (.7, 1.)]
        a["Ncut_factor"] = [(0, 0.), (2. / 3, 1.)]
        a["anneal_prior"] = False
        a.as_dict = lambda: {k: a[k] for k in ("T", "Ncut_factor")}
        params, out = dict(p0), []
        for _ in range(4):
            params = m.step(a, params, {"y": Y[:Nt]})
            out.append({k: np.array(v, copy=True) for k, v in params.items()})
            if interleave:
                res = m.inference(T1, {k: np.array(v, copy=True) for k, v in params.items()}, {"y": Y[Nt:]}, exact=True)
                assert res["s"].shape == (40, 10, H) and (m.Hprime, m.gamma) == (5, 3)
            a.next()
        return out
    for pa, pb in zip(train(False), train(True)):
        for k in pa:
            np.testing.assert_array_equal(pa[k], pb[k], err_msg=k)


# ------------------------------------------------------------------------------------------------------------ 6: refusals
@pytest.mark.parametrize("name", MODELS)
def test_refusals_before_any_launch(dev, name):
    from prosper_amd import _lib
    m, p, Y, _ = _case(name, 6)
    calls = _entries(m)
    try:
        with pytest.raises(NotImplementedError):
            m.inference(_An(T=1.3), p, {"y": Y}, exact=True)
        with pytest.raises(ValueError):
            m.inference(T1, p, {"y": Y}, exact=True, Hprime_max=6)
        with pytest.raises(ValueError):
            m.inference(T1, p, {"y": Y}, exact=True, gamma_max=6)
        for topK in (-1, 0, IR.MAX_TOPK + 1):
            with pytest.raises(ValueError):
                m.inference(T1, p, {"y": Y}, topK=topK, exact=True)
        for key in ("mask", "weight"):
            with pytest.raises(NotImplementedError, match="exact"):
                m.inference(T1, p, {"y": Y, key: np.ones_like(Y)}, exact=True)
    finally:
        del m._call
    assert not calls, calls
    big, pb, Yb, _, _ = _problem(name, np.random.RandomState(3), D, 33, 3, 3, 2)
    calls = _entries(big)
    with pytest.raises(_lib.HipError):
        big.inference(T1, pb, {"y": Yb}, exact=True)
    assert not calls, calls


@pytest.mark.parametrize("name", ["dsc", "tsc", "gsc_scalar"])
def test_other_models_refuse_by_name(dev, name):
    m, p, Y, _, _ = _problem(name, np.random.RandomState(3), D, 5, 4, 3, 2)
    calls = _entries(m)
    with pytest.raises(NotImplementedError, match=type(m).__name__):
        m.inference(T1, p, {"y": Y}, exact=True)
    assert not calls, calls
