"""reconstruct() without a GPU: the public method and the new C-ABI entries exist in the header, the binding
and both libraries; the entries reject bad arguments before they touch a device; and the NumPy restatements the GPU tests
compare against (tests/recon_reference.py) agree with each other."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import recon_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pm_recon_expect_f64", "pm_recon_mca_f64", "pm_gemm_nt_rows_f64")


def test_every_model_has_reconstruct():
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    from prosper_amd.em.camodels.mca_et import MCA_ET
    from prosper_amd.em.camodels.mmca_et import MMCA_ET
    from prosper_amd.em.camodels.dsc_et import DSC_ET
    from prosper_amd.em.camodels.tsc_et import TSC_ET
    from prosper_amd.em.camodels.gsc_et import GSC
    from prosper_amd.em.mixturemodels.MoG import MoG
    from prosper_amd.em.mixturemodels.MoP import MoP
    for cls in (BSC_ET, MCA_ET, MMCA_ET, DSC_ET, TSC_ET, GSC, MoG, MoP):
        assert callable(getattr(cls, "reconstruct", None)), cls.__name__
        doc = cls.reconstruct.__doc__
        assert doc and "device=True" in doc, cls.__name__
    assert "pseudo-states" in TSC_ET.reconstruct.__doc__          # the caveat log_likelihood carries
    assert "normalised" in MoP.reconstruct.__doc__                # the units of MoP's result


def test_new_entries_in_header_binding_and_both_libraries():
    from prosper_amd import _lib
    header = open(os.path.join(ROOT, "include", "prosper_hip.h")).read()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.SIGNATURES, name
    for path in (_lib.LIB_PATH, _lib.LIB_PATH_DET):
        lib = C.CDLL(path)
        for name in NEW:
            assert hasattr(lib, name), (path, name)
    assert _lib.load().pm_version() >= 1018 and _lib.MIN_VERSION >= 1018


PM_EINVAL, PM_ERANGE = -1, -2


@pytest.mark.parametrize("det", [False, True])
def test_entries_reject_bad_arguments_without_a_device(det):
    """Every pointer below is host memory (or NULL): a launch would fault, a correct entry returns before one."""
    from prosper_amd import _lib
    lib = _lib.load(det)
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    one = (C.c_double * 8)(1.0)

    def expect(logpj=p, ld=10, lse=None, a=1.0, off=None, cand=p, vals=p, bv=one, N=4, H=4, Hp=2, K=9, soff=1, nblk=1,
               moff=5, S=4, out=p, ldo=8, cols=8, ones=-1):
        return lib.pm_recon_expect_f64(logpj, ld, lse, a, off, cand, vals, bv, N, H, Hp, K, soff, nblk, moff, S, out, ldo,
                                       cols, ones, None)
    assert expect(logpj=None) == PM_EINVAL and expect(out=None) == PM_EINVAL
    assert expect(cand=None) == PM_EINVAL and expect(vals=None) == PM_EINVAL and expect(bv=None) == PM_EINVAL
    assert expect(N=-1) == PM_EINVAL and expect(H=0) == PM_EINVAL and expect(ld=8) == PM_EINVAL
    assert expect(ldo=7) == PM_EINVAL and expect(cols=3) == PM_EINVAL
    assert expect(ones=2) == PM_EINVAL and expect(ones=8) == PM_EINVAL
    assert expect(moff=6) == PM_EINVAL and expect(nblk=3) == PM_EINVAL          # columns past K
    assert expect(lse=p, a=0.5) == PM_EINVAL and expect(lse=p, off=p) == PM_EINVAL
    assert expect(Hp=17) == PM_ERANGE and expect(nblk=9, K=200, ld=200) == PM_ERANGE
    assert expect(N=0, logpj=None, out=None) == 0                              # nothing to do: no launch

    def mca(logpj=p, ld=100, cand=p, masks=p, Wrho=p, inv_rho=1 / 21., N=4, H=4, D=10, Hp=2, S=1, Y=p, ldy=None):
        return lib.pm_recon_mca_f64(logpj, ld, None, cand, masks, Wrho, inv_rho, 0, N, H, D, Hp, S, Y, D if ldy is None else ldy,
                                    None)
    for k in ("logpj", "cand", "masks", "Wrho", "Y"):
        assert mca(**{k: None}) == PM_EINVAL, k
    assert mca(N=-1) == PM_EINVAL and mca(ld=5) == PM_EINVAL and mca(ldy=9) == PM_EINVAL and mca(inv_rho=0.0) == PM_EINVAL
    assert mca(D=1025, ldy=1025) == PM_ERANGE and mca(Hp=17) == PM_ERANGE
    assert mca(N=0, logpj=None) == 0

    def gemm(A=p, B=p, Cc=p, M=4, N=4, K=8, lda=8):
        return lib.pm_gemm_nt_rows_f64(A, lda, B, 8, Cc, 8, M, N, K, None)
    assert gemm(A=None) == PM_EINVAL and gemm(B=None) == PM_EINVAL and gemm(Cc=None) == PM_EINVAL
    assert gemm(M=0) == PM_EINVAL and gemm(lda=7) == PM_EINVAL
    assert gemm(M=2 ** 31) == PM_ERANGE


def test_bsc_oracle_log_joints_at_full_state_set_give_the_enumerated_mean():
    """The weights rebuilt from the oracle E-step's (logpj, candidates) at H' = gamma = H and the plain enumeration of all
    2^H states are the same posterior mean: pins linear_from_lpj (column layout, candidate scatter) and enum_linear
    against each other, with and without mu."""
    from oracle import bsc_oracle as O
    rng = np.random.RandomState(3)
    D, H, N = 9, 5, 60
    W, pi, sigma = rng.normal(size=(D, H)), 0.3, 0.9
    for mu in (np.zeros(D), rng.normal(size=D)):
        Y = (rng.uniform(size=(N, H)) < pi) @ W.T + mu + sigma * rng.normal(size=(N, D))
        model = O.make_model(D, H, H, H)
        cand = O.select_hprimes_vec(W, Y - mu, H)
        logpj = O.e_step_vec(O.Anneal(T=1.0), W, pi, sigma, mu, Y, cand, model['SM'], model['state_abs'])
        assert logpj.shape == (N, 2 ** H)
        got = R.linear_from_lpj(logpj, 1.0, cand, W, (1.0,), 1, 1 + H, model['SM'], mu=mu)
        want = R.enum_linear(Y, W, sigma, [0., 1.], np.log([1 - pi, pi]), mu=mu)
        assert R.row_rel_err(got, want) < 1e-12


def test_tsc_oracle_log_joints_on_rows_with_distinct_candidates():
    """TSC at H' = H: on the rows whose candidates are distinct the table states are every state of the model once; the
    repeated-candidate rows hold pseudo-states and are left out (at most half, as the GPU test asserts)."""
    from oracle import tsc_oracle as O
    rng = np.random.RandomState(205)
    D, H, N = 9, 5, 200
    W, pi, sigma = rng.normal(size=(D, H)), 0.3, 0.8
    S = rng.choice(3, p=[pi / 2, 1 - pi, pi / 2], size=(N, H)) - 1.
    Y = S @ W.T + sigma * rng.normal(size=(N, D))
    model = O.make_model(D, H, H, H)
    cand = np.asarray(O.select_hprimes_vec(model, W, pi, sigma, Y))
    full = np.array([len(set(c)) == H for c in cand])
    assert full.sum() >= N // 2
    from oracle.bsc_oracle import Anneal
    SM = np.asarray(model['SM'], dtype=np.float64)
    logpj = O.e_step_vec(Anneal(T=1.0), model, W, pi, sigma, Y, cand)
    assert logpj.shape == (N, len(SM))
    got = R.linear_from_lpj(logpj, 1.0, cand, W, (), 0, 0, SM)
    want = R.enum_linear(Y, W, sigma, [-1., 0., 1.], np.log([pi / 2, 1 - pi, pi / 2]))
    assert R.row_rel_err(got[full], want[full]) < 1e-12
    # a row with a repeated candidate: the pseudo-state mean differs from the model's posterior mean
    assert (~full).any() and R.row_rel_err(got[~full], want[~full]) > 1e-6


def test_gsc_and_mca_restatements_agree_with_enumeration():
    """gsc_from_lpj / mca_from_lpj on hand-built log-joints over the full candidate set against enum_gsc / enum_mca."""
    import itertools
    rng = np.random.RandomState(5)
    D, H, N = 7, 4, 25
    SM = np.array([[1 if j in c else 0 for j in range(H)] for g in range(2, H + 1)
                   for c in itertools.combinations(range(H), g)])
    cand = np.tile(np.arange(H), (N, 1))
    sets = [[]] + [[h] for h in range(H)] + [list(np.nonzero(r)[0]) for r in SM]
    # MCA
    W, pi, sigma = rng.uniform(0.2, 3.0, size=(D, H)), 0.3, 0.7
    Y = rng.uniform(0, 3, size=(N, D))
    mean = R.mca_mean(W, 21.0, False)
    means = np.array([mean(a) for a in sets])
    logpj = np.array([len(a) for a in sets])[None, :] * np.log(pi / (1 - pi)) \
        - 0.5 * ((Y[:, None, :] - means[None]) ** 2).sum(-1) / sigma ** 2
    assert R.row_rel_err(R.mca_from_lpj(logpj, cand, SM, W, 21.0, False), R.enum_mca(Y, W, 21.0, False, pi, sigma)) < 1e-12
    # GSC: logpj holds TWICE the log-joint (the doubled-logit pass), read with a = 1/2
    Q = rng.normal(size=(H, H)) * 0.2
    p = {"W": rng.normal(size=(D, H)), "pi": rng.uniform(0.2, 0.4, size=H), "mu": rng.normal(size=H),
         "psi_sq": np.diag(rng.uniform(0.5, 1.5, size=H)) + Q @ Q.T, "sigma_sq": rng.uniform(0.4, 1.0, size=D)}
    Y = rng.normal(size=(N, D))
    logpj = 2.0 * np.stack([R.gsc_state_terms(p, Y, a)[0] for a in sets], axis=1)
    assert R.row_rel_err(R.gsc_from_lpj(p, Y, logpj, cand, SM), R.enum_gsc(p, Y)) < 1e-12


def test_expect_from_lpj_with_scale_and_offset_and_repeated_candidates():
    """E[s] under softmax(a X + off), written out column by column: one-cause blocks, table states scattered to their
    candidates (a repeated latent receives both positions), weight-only columns."""
    rng = np.random.RandomState(31)
    N, H, Hp = 5, 6, 3
    blocks = (-1.0, 2.0)
    table = rng.choice([-1.0, 0.0, 1.0], size=(4, Hp))
    soff, moff = 2, 2 + 2 * H
    K = moff + 4 + 1                                   # two leading and one trailing column carry weight only
    X, off, a = rng.normal(size=(N, K)), rng.normal(size=K), 0.7
    cand = np.array([rng.permutation(H)[:Hp] for _ in range(N)])
    cand[1] = [4, 4, 2]
    got = R.expect_from_lpj(X, a, cand, H, blocks, soff, moff, table, off=off)
    Z = a * X + off[None, :]
    q = np.exp(Z - Z.max(1, keepdims=True))
    q /= q.sum(1, keepdims=True)
    want = np.zeros((N, H))
    for n in range(N):
        for h in range(H):
            want[n, h] = sum(v * q[n, soff + c * H + h] for c, v in enumerate(blocks))
            for j in range(Hp):
                if cand[n, j] == h:
                    want[n, h] += sum(q[n, moff + s] * table[s, j] for s in range(4))
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=1e-15)
    W = rng.normal(size=(7, H))
    np.testing.assert_allclose(R.linear_from_lpj(X, 1.0, cand, W, blocks, soff, moff, table),
                               R.expect_from_lpj(X, 1.0, cand, H, blocks, soff, moff, table) @ W.T, rtol=1e-14)


@pytest.mark.parametrize("signed,rho", [(False, 21.0), (True, 6.0), (False, 3.5)])
def test_mca_multi_from_lpj_is_the_multi_cause_part_of_mca_from_lpj(signed, rho):
    from prosper_amd.em.camodels import generate_state_matrix
    from scipy.special import logsumexp
    rng = np.random.RandomState(32)
    N, D, H, Hp = 6, 9, 7, 4
    SM = generate_state_matrix(Hp, 3)[2]
    W = rng.uniform(0.2, 3.0, size=(D, H)) * (rng.choice([-1.0, 1.0], size=(D, H)) if signed else 1.0)
    lp = rng.normal(size=(N, 1 + H + len(SM)))
    cand = np.array([rng.permutation(H)[:Hp] for _ in range(N)])
    Wrho = (np.sign(W) * np.abs(W) ** rho).T
    multi = R.mca_multi_from_lpj(lp, logsumexp(lp, axis=1), cand, SM, Wrho, rho, signed)
    whole = R.mca_from_lpj(lp, cand, SM, W, rho, signed)
    np.testing.assert_allclose(R.softmax_rows(lp)[:, 1:1 + H] @ W.T + multi, whole, rtol=1e-12, atol=1e-13)


def test_dsc_state_table_equals_the_references_enumeration():
    """DSC_ET's table of multi-cause states is built from the non-zeros' positions and values; it must be the array the
    reference's filter over all K^Hprime vectors gives (dsc_et.py:56-63), order and dtype included -- and H' = 12 with four
    latent values (test_against_the_esteps_log_joints[dsc4-24-130-12-2]) must not take minutes."""
    import itertools
    import time
    from prosper_amd.em.camodels.dsc_et import get_states

    def reference(states, Hprime, gamma):
        sl = [np.array(c) for c in itertools.product(states, repeat=Hprime)
              if (np.sum(np.array(c) != 0) <= gamma and np.sum(np.array(c) != 0) > 1)]
        return np.array(sl) if sl else np.zeros((0, Hprime))
    for states in (np.array([0, 1]), np.array([-1., 0., 1.]), np.array([0., 1., 2., 3.]),
                   np.array([-3., -2., -1., 0., 1., 2., 3., 4.]), np.array([1., 2.]), np.array([0., 0., 1.])):
        for Hp, g in ((1, 1), (2, 1), (2, 2), (3, 2), (4, 3), (5, 2), (5, 5), (6, 4)):
            if len(states) ** Hp > 40000:
                continue
            want, got = reference(states, Hp, g), get_states(states, Hp, g)
            assert got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want), (states, Hp, g)
    t = time.time()
    table = get_states(np.array([0., 1., 2., 3.]), 12, 2)
    assert table.shape == (66 * 9, 12) and time.time() - t < 5.0

