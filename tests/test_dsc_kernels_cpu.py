"""tests/dsc_kernels_reference.py pinned without a device: its statements of the DSC / TSC selection, E-step and M-step
statistics against oracle/dsc_oracle.py and oracle/tsc_oracle.py (the per-datapoint loops of the reference implementation)
at small real-valued shapes, to 1e-12 relative; the dispatch table of tests/test_dsc_kernels_gpu.py against pm_dsc_plan (a
host-only query: the launchers switch on the same function); and the two properties of that module's data its comparisons
rest on -- the arithmetic is exact, and in the hot cases every posterior weight of a row is above 1 / (e Kt)."""
import ctypes

import numpy as np
import pytest

import dsc_kernels_reference as R
from oracle import dsc_oracle as DO
from oracle import tsc_oracle as TO

PM_EINVAL, PM_ERANGE = -1, -2
RTOL = 1e-12


def _close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale = np.abs(want).max() if want.size else 1.0
    assert np.abs(got - want).max() <= RTOL * max(scale, 1e-300), (what, float(np.abs(got - want).max()), float(scale))


def _abi_inputs(W_DH, Y):
    W = W_DH.T
    return Y @ W.T, W @ W.T, (Y * Y).sum(axis=1)


# ------------------------------------------------------------------------------------------------- against the oracles
@pytest.mark.parametrize("D,H,Hp,gamma,states,T,prior_anneal,ncut", [
    (7, 6, 3, 2, (0., 1., 2.), 1.0, False, 0.0),
    (5, 5, 4, 3, (-1., 0., 1.5), 1.3, True, 0.0),
    (6, 7, 3, 3, (2., -1., 0., 0.5), 1.2, False, 0.6),
    (4, 4, 2, 1, (0., 1.), 1.0, False, 0.0)])
def test_reference_matches_the_dsc_oracle(D, H, Hp, gamma, states, T, prior_anneal, ncut):
    rng = np.random.RandomState(D + H)
    model = DO.make_model(D, H, Hp, gamma, states)
    K, K0, S = model['K'], model['K_0'], model['no_states']
    W_DH = rng.normal(size=(D, H))
    N = 23
    Y = rng.normal(size=(N, D)) * 1.5
    pi = rng.dirichlet(np.ones(K) * 3)
    sigma = 0.9
    anneal = DO.Anneal(T=T, Ncut_factor=ncut, anneal_prior=prior_anneal)
    A, G, yn = _abi_inputs(W_DH, Y)
    values = np.asarray(states, dtype=np.float64)
    pre1 = -0.5 / sigma ** 2
    # selection
    cand = DO.select_hprimes_loop(model, W_DH, pi, sigma, Y)
    assert np.array_equal(R.dsc_candidates(A, G, values, K0, np.log(pi), pre1, Hp), cand)
    _close(-R.dsc_select_scores(A, G, values, K0, np.log(pi), pre1), DO.select_scores_vec(model, W_DH, pi, sigma, Y), "R")
    # E-step: columns [null | singletons by value then latent | states]
    state_idx = np.array([[int(np.argwhere(values == v)[0, 0]) for v in row] for row in model['SM']],
                         dtype=np.uint8).reshape(S, Hp)
    beta = 1.0 / T
    prior = DO.prior_terms(model, pi)
    E = R.energies(A, G, yn, cand, values, K0, state_idx, 0)
    F = R.log_joints(E, prior, pre1 * beta, beta if prior_anneal else 1.0)
    want = DO.e_step_loop(anneal, model, W_DH, pi, sigma, Y, cand)
    _close(F, want, "logpj")
    # M-step
    l = R.lse(want)
    _close(l, np.log(np.exp(want).sum(axis=1)), "lse")
    _, log = DO.m_step(anneal, model, W_DH, pi, sigma, Y, cand, want)
    keep = np.ones(N, dtype=bool)
    if ncut > 0:
        n_use = int(N * (1 - (1 - log['prior_mass']) * ncut))
        keep = np.asarray(l > np.sort(l)[-n_use])                     # strict
    assert log['N_use'] == keep.sum()
    st = R.row_stats(want, l, keep, E, cand, values, K0, state_idx, 0, H, D)
    stats = st["stats"]
    _close(st["expect"].T.astype(np.float64) @ Y, log['stats']['Wp'], "Wp")
    Wq = stats[H * D:H * D + H * H].reshape(H, H) + np.diag(stats[H * D + H * H:H * D + H * H + H])
    _close(Wq, np.triu(log['stats']['Wq']), "Wq")
    assert not np.tril(Wq, -1).any()
    cnt = stats[H * D + H * H + H:H * D + H * H + H + R.MAX_K]
    for k in range(K):
        if k != K0:
            _close(cnt[k], log['stats']['pi'][k], "count %d" % k)
    assert cnt[K0] == 0 and not cnt[K:].any()
    scal = stats[-4:]
    _close(scal[0] / D, log['stats']['sigma'], "sigma")
    _close(scal[1] / keep.sum(), log['L'] + 0.5 * D * np.log(2 * np.pi * sigma ** 2), "L")
    assert scal[2] == keep.sum()
    assert np.array_equal(st["expect"][~keep], np.zeros((int((~keep).sum()), H)))


@pytest.mark.parametrize("D,H,Hp,gamma,T,prior_anneal", [(6, 5, 3, 2, 1.0, False), (5, 4, 4, 3, 1.4, True), (7, 6, 5, 2, 1.1, False)])
def test_reference_matches_the_tsc_oracle(D, H, Hp, gamma, T, prior_anneal):
    rng = np.random.RandomState(3 * D + H)
    model = TO.make_model(D, H, Hp, gamma)
    W_DH = rng.normal(size=(D, H))
    N = 29
    Y = rng.normal(size=(N, D)) * 1.5
    pi, sigma = 0.3, 1.1
    anneal = TO.Anneal(T=T, Ncut_factor=0.0, anneal_prior=prior_anneal)
    A, G, yn = _abi_inputs(W_DH, Y)
    values, K0 = TO.STATES, 1
    cand = TO.select_hprimes_loop(model, W_DH, pi, sigma, Y)
    assert np.array_equal(R.tsc_candidates(A, G, Hp), cand)
    assert any(len(set(c)) < Hp for c in cand.tolist())               # latents repeat: the last-position rule matters below
    _close(R.tsc_select_scores(A, G), TO.select_scores_vec(model, W_DH, Y), "R")
    assert np.array_equal(np.stack([R.last_positions(c) for c in cand]), TO.last_position_mask(cand))
    SM = model['SM']
    state_idx = (SM.astype(np.int64) + 1).astype(np.uint8)
    flags = R.TABLE_ONLY | R.LAST_POSITION
    beta = 1.0 / T
    pre1 = -0.5 / sigma ** 2
    E = R.energies(A, G, yn, cand, values, K0, state_idx, flags)
    F = R.log_joints(E, TO.log_prior(SM, pi), pre1 * beta, beta if prior_anneal else 1.0)
    want = TO.e_step_loop(anneal, model, W_DH, pi, sigma, Y, cand)
    _close(F, want, "logpj")
    l = R.lse(want)
    _, log = TO.m_step(anneal, model, W_DH, pi, sigma, Y, cand, want)
    st = R.row_stats(want, l, np.ones(N, dtype=bool), E, cand, values, K0, state_idx, flags, H, D)
    stats = st["stats"]
    _close(st["expect"].T.astype(np.float64) @ Y, log['stats']['Wp'], "Wp")
    _close(stats[H * D:H * D + H * H].reshape(H, H), np.triu(log['stats']['Wq']), "Wq")
    assert not stats[H * D + H * H:H * D + H * H + H].any()           # no singleton columns: qdiag stays zero
    cnt = stats[H * D + H * H + H:H * D + H * H + H + R.MAX_K]
    _close(cnt[0] + cnt[2], log['stats']['pi'], "pi")
    _close(stats[-4], log['stats']['sigma'], "sigma")
    assert stats[-2] == N


def test_ranking_tie_rules():
    """Equal values: smallest-first keeps the smaller index first; largest (best last) puts the larger index last."""
    Rm = np.array([[3., 1., 1., 0., 3., 1.]])
    assert R.rank_smallest_first(Rm, 3).tolist() == [[3, 1, 2]]
    assert R.rank_largest_best_last(Rm, 3).tolist() == [[5, 0, 4]]


def test_lists_and_overflow():
    """Non-zero lists: ascending latents, the first sixteen kept, 0xFFFF behind them, overflowing rows counted."""
    H, D = 18, 1
    values, K0 = np.array([0., 1.]), 0
    F = np.log(np.array([[1.] + [1.] * 16 + [0., 0.], [1.] + [1.] * 17 + [0.], [1.] + [0.] * 17 + [1.]]) + 1e-300)
    l = R.lse(F)
    st = R.row_stats(F, l, [True, True, False], np.zeros_like(F), np.zeros((3, 1), dtype=int), values, K0,
                     np.zeros((0, 1), dtype=np.uint8), 0, H, D)
    assert st["nz_cnt"].tolist() == [18, 18, 0]                       # (the 1e-300 weights are non-zero in longdouble)
    assert st["nz_idx"][0].tolist() == list(range(16)) and st["nz_idx"][2].tolist() == [R.NZ_PAD] * 16
    assert st["stats"][-1] == 2 and st["stats"][-2] == 2


# ------------------------------------------------------------------------------------------------------- the plan table
def _plan(lib, which, H, Hp, S, K, flags, N):
    out = (ctypes.c_int32 * 8)(*([-7] * 8))
    rc = lib.pm_dsc_plan(which, H, Hp, S, K, flags, N, out)
    return rc, list(out)


def _libs():
    from prosper_amd import _lib
    return [_lib.load(False), _lib.load(True)]


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_plan_of_every_case(name):
    """Every case of the GPU module takes the path its table says, in both libraries; the _supported queries agree with
    the plan; a sweep case has N past two full grid sweeps of every entry (and at most one sweep of rows past the largest)."""
    H, Hp, K, K0, S, N, D, flags, kind = R.CASES[name][:9]
    for lib in _libs():
        sweeps = []
        for which in (R.ESTEP, R.MSTATS, R.ROWS):
            want = R.CASES[name][9 + which]
            rc, out = _plan(lib, which, H, Hp, S, K, flags, N)
            if want is None:
                assert rc == PM_ERANGE and out == [-7] * 8, (name, which, rc, out)
                continue
            assert rc == 0 and tuple(out[:6]) == want, (name, which, rc, out)
            per_group = 16 if out[0] == R.L16 else 4
            assert out[7] == min(-(-N // per_group), out[7]) and 0 < out[6] <= 64 * 1024, (name, which, out)
            sweeps.append(out[7] * per_group)
        assert bool(lib.pm_dsc_estep_mstats_supported(H, Hp, S, K, flags)) == (R.CASES[name][9 + R.MSTATS] is not None)
        assert bool(lib.pm_dsc_rows16_supported(H, Hp, S, K, flags)) == (R.CASES[name][9 + R.ROWS][0] == R.L16)
        if N > 1000:
            assert H <= 17 and D <= 3 and all(N > 2 * s for s in sweeps) and N < 2 * max(sweeps) + 16, (name, N, sweeps)
        else:
            assert all(N <= s for s in sweeps)


def test_plan_table_covers_every_cell_and_edge():
    cells = {w: set() for w in (R.ESTEP, R.MSTATS, R.ROWS)}
    for c in R.CASES.values():
        for w in cells:
            if c[9 + w] is not None:
                cells[w].add(c[9 + w])
    for w in cells:
        fam = {(p[0], p[1], p[2]) for p in cells[w]}
        assert {(R.L16, 8, 8), (R.L16, 8, 16), (R.L16, 16, 8), (R.L16, 16, 16)} <= fam, (w, fam)
        assert {p[4] for p in cells[w]} == {0, 1}, w                                        # stage on and off
        if w != R.MSTATS:
            assert {(R.WAVE, 8, 0), (R.WAVE, 16, 0)} <= fam, (w, fam)
    assert {(p[1], p[2], p[3]) for p in cells[R.MSTATS]} >= {(m, v, k) for m in (8, 16) for v in (8, 16) for k in (4, 8)} - \
        {(16, 8, 8), (8, 16, 8)}                                                            # KM = 8 at <8,8> and <16,16>
    for w in (R.ESTEP, R.MSTATS):
        assert any(p[5] > 0 for p in cells[w]) and any(p[5] == 0 for p in cells[w])
    shapes = [c[:9] for c in R.CASES.values()]
    col = lambda i: {s[i] for s in shapes}
    assert col(0) >= {1, 15, 16, 17, 128, 129, 256, 257} and col(1) >= {1, 2, 4, 8, 9, 16}
    assert col(2) >= {2, 3, 4, 5, 8} and col(4) >= {0, 1, 15, 16, 17} and col(5) >= {1, 15, 16, 17, 67} and col(6) == {1, 3}
    assert any(s[3] == 0 for s in shapes) and any(s[3] == s[2] - 1 for s in shapes) and any(0 < s[3] < s[2] - 1 for s in shapes)
    # NT = 0 for each of its reasons: S = 0; the count past 256 (K = 5, H' = 6)
    assert R.CASES["s0"][4] == 0 and R.CASES["s0"][9][5] == 0
    H, Hp, K = R.CASES["km8_nt_over"][:3]
    assert 1 + Hp * (K - 1) + Hp * (Hp - 1) // 2 * (K - 1) ** 2 > 256 and R.CASES["km8_nt_over"][9][5] == 0
    # wave kernels through H > 256 and, at H <= 256, through the LDS size
    for w in (R.ESTEP, R.ROWS):
        for hp in (8, 16):
            hs = {c[0] for c in R.CASES.values() if c[9 + w] is not None and c[9 + w][:2] == (R.WAVE, hp)}
            assert any(h > 256 for h in hs) and any(h <= 256 for h in hs), (w, hp, hs)
    # the four-non-zero state of the "four" tables sits beside a table without one
    for name in ("too_many", "too_many_wave", "le3"):
        c = R.make_case(name, True)
        nnz = (c["state_idx"] != c["K0"]).sum(axis=1)
        assert nnz.max() == (3 if name == "le3" else 4) and R.CASES[name][9][5] > 0


def test_plan_rejects_what_the_launchers_reject():
    from prosper_amd import _lib
    assert _lib.load().pm_version() >= 1022 and _lib.MIN_VERSION >= 1022
    for lib in _libs():
        out = (ctypes.c_int32 * 8)(*([-7] * 8))
        assert lib.pm_dsc_plan(0, 17, 3, 7, 3, 0, 16, None) == PM_EINVAL
        for bad in [(3, 17, 3, 7, 3, 0, 16), (-1, 17, 3, 7, 3, 0, 16), (0, 0, 3, 7, 3, 0, 16), (0, 17, 0, 7, 3, 0, 16),
                    (0, 17, 3, -1, 3, 0, 16), (0, 17, 3, 7, 1, 0, 16), (0, 17, 3, 7, 9, 0, 16), (0, 17, 3, 7, 3, 0, 0)]:
            assert lib.pm_dsc_plan(*bad, out) == PM_EINVAL, bad
        for big in [(0, 17, 18, 7, 3, 0, 16), (2, 3, 4, 7, 3, 0, 16), (1, 64, 17, 7, 3, 0, 16), (0, 65537, 3, 7, 3, 0, 16),
                    (1, 257, 3, 7, 3, 0, 16), (2, 65536, 16, 1 << 16, 3, 0, 16)]:
            assert lib.pm_dsc_plan(*big, out) == PM_ERANGE, big
        assert list(out) == [-7] * 8


# ------------------------------------------------------------------------------------------------ the data of the cases
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_case_arithmetic_is_exact_and_hot_weights_are_flat(name):
    """Energies are integers below 2^30 and ecoef e + pscale prior is exact in float64 (equal to the longdouble value:
    with or without a fused multiply-add, in any order of the energy's terms).  Hot: every weight above 1 / (e Kt), so one
    dropped, doubled or misplaced column moves a result by ~1 / Kt.  Cold: terms fall below the e^-37 / e^-60 cut-offs."""
    for hot in (True, False):
        c = R.make_case(name, hot)
        ref = R.case_reference(c)
        assert ref["exact"], (name, hot)
        assert c["ecoef"] in (-2.0, -2.0 ** -20) and c["pscale"] in (1.0, 0.5) and (c["prior"] * 16 == np.rint(c["prior"] * 16)).all()
        if c["Kt"] == 0:
            continue
        r = c["rows"]
        d = ref["F"][:r] - ref["F"][:r].max(axis=1)[:, None]
        if hot:
            q = R.weights(ref["F"][:r], ref["lse"][:r])
            assert q.min() > 1.0 / (np.e * c["Kt"]), (name, float(q.min()), c["Kt"])
        elif name != "h1":
            assert (d < -37).any() and (d - np.log(np.exp(d).sum(axis=1))[:, None] < -60).any(), name
        if not c["flags"] & R.LAST_POSITION:
            assert all(len(set(x)) == c["Hp"] for x in c["cand"][:r].tolist())
        else:
            assert any(len(set(x)) < c["Hp"] for x in c["cand"][:r].tolist()) or c["Hp"] == 1
        assert c["cand"].min() >= 0 and c["cand"].max() < c["H"] and c["state_idx"].max(initial=0) < c["K"]
