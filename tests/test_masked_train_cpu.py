"""The NumPy restatement of the masked BSC EM step (tests/masked_train_reference.py) pinned on the CPU: against
the reference's own goldens at an all-ones mask, against the oracle's unmasked step on the sub-model when every row shares
one mask, and as an exact EM whose free energy never decreases."""
import numpy as np

from conftest import golden
from oracle import bsc_oracle as O

import masked_train_reference as T

RTOL_STEP = 1e-8


def _golden_step(case):
    g = golden(case + ".npz")
    an = T.Anneal(T=float(g["T"]), anneal_prior=bool(g["anneal_prior"]))
    params = {"W": g["W"], "pi": float(g["pi"]), "sigma": float(g["sigma"]), "mu": g["mu"]}
    new, log = T.step(an, params, g["y"], np.ones_like(g["y"], dtype=bool), int(g["Hprime"]), int(g["gamma"]))
    return g, new, log


def test_all_ones_mask_equals_the_reference_goldens():
    for case in ("bsc_step_c1_plain", "bsc_step_h32"):
        g, new, log = _golden_step(case)
        assert np.array_equal(np.sort(log["cand"], axis=1), np.sort(g["candidates"], axis=1))
        scale = np.abs(g["W_new"]).max()
        errW = np.abs(new["W"] - g["W_new"]).max() / scale
        print("%s: W %.2e pi %.2e sigma %.2e L %.2e" % (case, errW, abs(new["pi"] / g["pi_new"] - 1),
                                                      abs(new["sigma"] / g["sigma_new"] - 1), abs(log["L"] / g["L"] - 1)))
        np.testing.assert_allclose(new["W"], g["W_new"], rtol=RTOL_STEP, atol=RTOL_STEP * scale)
        np.testing.assert_allclose(new["pi"], g["pi_new"], rtol=RTOL_STEP)
        np.testing.assert_allclose(new["sigma"], g["sigma_new"], rtol=RTOL_STEP)
        np.testing.assert_allclose(log["L"], g["L"], rtol=1e-11)
        assert log["W_kept"] == 0 and log["N"] == int(g["N"])


def test_shared_mask_equals_the_oracle_on_the_sub_model():
    rng = np.random.RandomState(5)
    D, H, Hp, gamma, N = 20, 8, 5, 3, 150
    params, Y, _ = T.model_problem(rng, D, H, N, never=False)
    obs = np.sort(rng.permutation(D)[:12])
    M = np.zeros((N, D), dtype=bool)
    M[:, obs] = True
    an = T.Anneal(T=1.3, anneal_prior=True)
    new, log = T.step(an, params, np.where(M, Y, np.nan), M, Hp, gamma)
    oan = O.Anneal(T=1.3, anneal_prior=True)
    sub = {"W": params["W"][obs], "pi": params["pi"], "sigma": params["sigma"]}
    ref, rlog = O.em_step(oan, O.make_model(len(obs), H, Hp, gamma), sub, Y[:, obs], stats_fn=O.m_step_stats_vec, vec=True)
    assert np.array_equal(log["cand"], rlog["candidates"])
    scale = np.abs(ref["W"]).max()
    np.testing.assert_allclose(new["W"][obs], ref["W"], rtol=RTOL_STEP, atol=RTOL_STEP * scale)
    np.testing.assert_allclose([new["pi"], new["sigma"]], [ref["pi"], ref["sigma"]], rtol=RTOL_STEP)
    np.testing.assert_allclose(log["L"], rlog["L"], rtol=1e-11)
    rest = np.setdiff1d(np.arange(D), obs)
    assert np.array_equal(new["W"][rest], params["W"][rest])            # unobserved rows of W are kept
    assert log["W_kept"] == len(rest) and np.array_equal(np.nonzero(log["kept"])[0], rest)


def test_exact_em_is_monotone():
    Ls, params = T.exact_em_trajectory()
    Ls = np.array(Ls)
    steps = np.diff(Ls)
    print("exact EM: L %.6f -> %.6f, smallest step %.3e, pi %.4f sigma %.4f" % (Ls[0], Ls[-1], steps.min(), params["pi"],
                                                                                 params["sigma"]))
    assert (Ls[1:] >= Ls[:-1] - 1e-10 * np.abs(Ls[:-1])).all(), steps.min()
    assert abs(params["pi"] - 0.2) < 0.03 and abs(params["sigma"] - 1.0) < 0.08
