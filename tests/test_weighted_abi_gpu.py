"""The weighted kernels (weighted_kernels.hip) through the C ABI -- pm_weighted_prepare_f64,
pm_bsc_weighted_estep_f64, pm_mca_weighted_select_scores_f64, pm_mca_weighted_estep_f64 -- on padded operands inside
pattern-filled buffers (the harness of tests/test_eval_kernels_gpu.py: guard rows, padding columns, inputs bit-unchanged).

Continuous data and weights (30 % zeros, the rest uniform in [0.25, 4]; a row of ones, a row of zeros), whatever the entries at
weight 0 hold: the outputs against NumPy at the project's 1e-11 row-relative; the BSC candidates equal the selection rule
applied to the same b and g (the reference's boundary gap asserted first).  Weights in {0, 1}: every entry returns the bits of
its masked counterpart on the same operands."""
import ctypes

import numpy as np
import pytest
from scipy.special import logsumexp

import masked_reference as MR
import weighted_reference as WR
from test_eval_kernels_gpu import (LAYOUTS, RTOL, Emb, _bsc_model, _ld, _mca_model, _mca_weights, _ok, _stream, emb_mask,
                                   garbage, row_rel)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GAP = 1e-9


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU box (MI355X)")
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def _weights(N, D, seed, binary=False):
    """Row 0 all ones, the last row all zeros (when there are at least three)."""
    rng = np.random.RandomState(seed)
    Om = np.where(rng.uniform(size=(N, D)) < 0.3, 0.0, 1.0 if binary else rng.uniform(0.25, 4.0, size=(N, D)))
    if N >= 3:
        Om[0] = 1.0
        Om[N - 1] = 0.0
    return Om


def _bits(a, b, what):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), what


# ------------------------------------------------------------------------------------------------ pm_weighted_prepare_f64
def _prepare(dev, Y, Om, mu, layout, with_x0=True):
    from prosper_amd import _lib
    N, D = Y.shape
    ey, eo = Emb(Y, _ld(D, layout, 0), dev), Emb(Om, _ld(D, layout, 1), dev)
    emu = Emb(mu, D, dev) if mu is not None else None
    exw, eom = Emb(Om, _ld(D, layout, 2), dev, fill=False), Emb(Om, _ld(D, layout, 3), dev, fill=False)
    ex0 = Emb(Om, _ld(D, layout, 4), dev, fill=False)
    en, elw = Emb(np.zeros(N), N, dev, fill=False), Emb(np.zeros(N), N, dev, fill=False)
    ed = Emb(np.zeros(N, dtype=np.int32), N, dev, fill=False)
    _lib.call("pm_weighted_prepare_f64", ey.ptr, ey.ld, eo.ptr, eo.ld, emu.ptr if emu is not None else None, N, D, exw.ptr,
              exw.ld, eom.ptr, eom.ld, ex0.ptr if with_x0 else None, ex0.ld, en.ptr, ed.ptr, elw.ptr, _stream())
    torch.cuda.synchronize()
    what = (N, D, mu is not None, layout, with_x0)
    assert all(e.outside_untouched() for e in (exw, eom, ex0, en, ed, elw)), what
    assert exw.written() and eom.written() and (ex0.written() if with_x0 else ex0.unchanged()), what
    assert _ok(ey, eo) and (emu is None or emu.unchanged()), what
    return exw.host(), eom.host(), ex0.host() if with_x0 else None, en.host()[0], ed.host()[0], elw.host()[0]


@pytest.mark.parametrize("D", [1, 63, 64, 65, 130])
def test_weighted_prepare(dev, D):
    """Xw, Om, X0 are one rounding each (Om and X0 exact); sum omega x^2 and sum log omega at 1e-11 of the sum of their terms'
    magnitudes; D_n exact.  N = 8197 rows reach the second trip of the row loop.  With omega in {0, 1}: the bits of
    pm_masked_prepare_f64."""
    from prosper_amd import _lib
    for N in (1, 5, 70) + ((8197,) if D == 1 else ()):
        rng = np.random.RandomState(N + D)
        Y0, Om = rng.normal(size=(N, D)) * 3, _weights(N, D, N * D + 1)
        Y = garbage(Y0, Om, N + 2 * D)
        for with_mu in (False, True):
            mu = rng.normal(size=D) if with_mu else None
            X = np.where(Om != 0, Y0 - (mu if with_mu else 0.0), 0.0)
            for k, layout in enumerate(LAYOUTS):
                xw, om, x0, xn2, dn, lw = _prepare(dev, Y, Om, mu, layout, with_x0=k % 2 == 0)
                what = (N, D, with_mu, layout)
                assert np.array_equal(xw, Om * X) and np.array_equal(om, Om), what
                assert x0 is None or np.array_equal(x0, X), what
                assert np.array_equal(dn, (Om != 0).sum(axis=1)), what
                want = (Om * X * X).sum(axis=1)
                assert (np.abs(xn2 - want) <= RTOL * np.abs(want)).all(), what
                with np.errstate(divide="ignore"):
                    logs = np.where(Om != 0, np.log(np.where(Om != 0, Om, 1.0)), 0.0)
                assert (np.abs(lw - logs.sum(axis=1)) <= RTOL * np.abs(logs).sum(axis=1)).all(), what
        # weights in {0, 1} against the masked entry, bit for bit
        B = _weights(N, D, N + 7 * D, binary=True)
        Yb = garbage(Y0, B, N + D + 3)
        mu = rng.normal(size=D)
        xw, om, x0, xn2, dn, lw = _prepare(dev, Yb, B, mu, "odd")
        ey, em, emu = Emb(Yb, D + 1, dev), emb_mask(B.astype(np.uint8), D + 2, dev), Emb(mu, D, dev)
        ex, ef = Emb(B, D, dev, fill=False), Emb(B, D + 3, dev, fill=False)
        en, ed = Emb(np.zeros(N), N, dev, fill=False), Emb(np.zeros(N, dtype=np.int32), N, dev, fill=False)
        _lib.call("pm_masked_prepare_f64", ey.ptr, ey.ld, em.ptr, em.ld, emu.ptr, N, D, ex.ptr, ex.ld, ef.ptr, ef.ld, en.ptr,
                  ed.ptr, _stream())
        torch.cuda.synchronize()
        _bits(xw, ex.host(), "Xw against the masked X0")
        _bits(x0, ex.host(), "X0")
        _bits(om, ef.host(), "Om against Mf")
        _bits(xn2, en.host()[0], "xnorm2")
        assert np.array_equal(dn, ed.host()[0]) and not lw.any()


# --------------------------------------------------------------------------------------- pm_mca_weighted_select_scores_f64
@pytest.mark.parametrize("H", [1, 63, 64, 65, 130])
def test_mca_weighted_select_scores(dev, H):
    """R[n,h] = sum_d omega_d max(W[h,d] - y_d, 0) at 1e-11 row-relative; 64 x 64 output tiles: H and N of 1, 63, 64, 65 and 130,
    D across the 16-wide slabs.  With omega in {0, 1}: the bits of pm_mca_masked_select_scores_f64."""
    from prosper_amd import _lib
    for N in (1, 63, 65):
        for D in (1, 15, 16, 17, 70):
            rng = np.random.RandomState(N + H + D)
            Y0, W = rng.uniform(0, 3, size=(N, D)), rng.uniform(0.1, 3, size=(H, D))
            for binary in (False, True):
                Om = _weights(N, D, N + H + D, binary)
                want = WR.score_mca(Y0, Om, W.T)
                for k, layout in enumerate(LAYOUTS if not binary else ["mix_a"]):
                    Y = garbage(Y0, Om, k) if k else np.where(Om != 0, Y0, 0.0)
                    ey, eo = Emb(Y, _ld(D, layout, 0), dev), Emb(Om, _ld(D, layout, 1), dev)
                    ew, er = Emb(W, _ld(D, layout, 2), dev), Emb(want, _ld(H, layout, 3), dev, fill=False)
                    _lib.call("pm_mca_weighted_select_scores_f64", ey.ptr, ey.ld, eo.ptr, eo.ld, ew.ptr, ew.ld, er.ptr, er.ld,
                              N, H, D, _stream())
                    torch.cuda.synchronize()
                    got = er.host()
                    assert row_rel(got, want) <= RTOL, (N, H, D, layout, row_rel(got, want))
                    assert er.outside_untouched() and er.written() and _ok(ey, eo, ew), (N, H, D, layout)
                if binary:
                    em, em_r = emb_mask(Om.astype(np.uint8), D + 1, dev), Emb(want, H, dev, fill=False)
                    _lib.call("pm_mca_masked_select_scores_f64", ey.ptr, ey.ld, em.ptr, em.ld, ew.ptr, ew.ld, em_r.ptr, em_r.ld,
                              N, H, D, _stream())
                    torch.cuda.synchronize()
                    _bits(got, em_r.host(), (N, H, D))


# ------------------------------------------------------------------------------------------- pm_bsc_weighted_estep_f64
def _run_bsc(dev, m, P, b, g, xn2, Om, Wt, layout, masked=False):
    from prosper_amd import _lib
    N, H = b.shape
    D, Hp, S = Wt.shape[1], m.Hprime, m.no_states
    K = 1 + H + S
    eb, eg = Emb(b, _ld(H, layout, 0), dev), Emb(g, _ld(H, layout, 1), dev)
    en, ew = Emb(xn2, N, dev), Emb(Wt, _ld(D, layout, 3), dev)
    eo = emb_mask(Om.astype(np.uint8), _ld(D, layout, 2), dev) if masked else Emb(Om, _ld(D, layout, 2), dev)
    ec = Emb(np.zeros((N, Hp), dtype=np.int32), Hp, dev, fill=False)
    el = Emb(np.zeros((N, K)), _ld(K, layout, 4), dev, fill=False)
    masks = m._state_tables()["masks"]
    _lib.call("pm_bsc_masked_estep_f64" if masked else "pm_bsc_weighted_estep_f64", eb.ptr, eb.ld, eg.ptr, eg.ld, en.ptr, eo.ptr,
              eo.ld, ew.ptr, ew.ld, ctypes.c_void_p(masks.data_ptr()), S, ctypes.byref(P), N, H, D, Hp, ec.ptr, el.ptr, el.ld,
              _stream())
    torch.cuda.synchronize()
    what = (H, D, Hp, layout)
    assert ec.outside_untouched() and el.outside_untouched() and ec.written() and el.written(), what
    assert _ok(eb, eg, en, eo, ew), what
    return ec.host(), el.host()


# (H, D, H', gamma): one H per latents-per-lane instantiation (VPL 1, 2, 4, 8, 16: H <= 64 VPL, PM_MAX_H = 1024 itself), H' of 12
# and 16 -- 66 and 120 candidate pairs, the second pair of a lane --, D below, at, one past and across the 64-wide slabs
BSC_SHAPES = [(61, 70, 5, 3), (125, 33, 12, 2), (253, 64, 6, 3), (509, 130, 5, 2), (1024, 40, 16, 2), (24, 65, 6, 3)]


@pytest.mark.parametrize("H,D,Hp,gamma", BSC_SHAPES)
def test_bsc_weighted_estep(dev, H, D, Hp, gamma):
    N = 9
    m, P = _bsc_model(D, H, Hp, gamma)
    rng = np.random.RandomState(H + D)
    Wt, X = rng.normal(size=(H, D)), rng.normal(size=(N, D)) * 2
    ppil = P.prior_scale * P.pil_bar
    SM = np.asarray(m.state_matrix, dtype=np.float64)
    for binary in (False, True):
        Om = _weights(N, D, H * D, binary)
        Xs = np.where(Om != 0, X, 0.0)
        b, g, xn2 = (Om * Xs) @ Wt.T, Om @ (Wt * Wt).T, (Om * Xs * Xs).sum(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            score = np.where(g > 0, b / np.sqrt(np.where(g > 0, g, 1.0)), 0.0)
        gap = MR.boundary_gap(score, Hp, True)[(Om != 0).any(axis=1)]
        assert (gap > GAP).all(), gap.min()
        want_c = MR.bsc_select_rule(b, g, Hp)
        size = np.concatenate([[0.0], np.ones(H), SM.sum(axis=1)])[None, :]
        e = np.empty((N, 1 + H + SM.shape[0]))
        e[:, 0] = xn2
        e[:, 1:1 + H] = g - 2.0 * b + xn2[:, None]
        for n in range(N):
            Wc = Wt[want_c[n]]
            G = (Wc * Om[n][None, :]) @ Wc.T
            G[np.diag_indices_from(G)] = g[n, want_c[n]]
            e[n, 1 + H:] = xn2[n] - 2.0 * (SM @ b[n, want_c[n]]) + np.einsum("si,ij,sj->s", SM, G, SM)
        want = ppil * size + P.ecoef * e
        for layout in (LAYOUTS if not binary else ["odd"]):
            cand, logpj = _run_bsc(dev, m, P, b, g, xn2, Om, Wt, layout)
            assert np.array_equal(cand, want_c), (H, layout, np.argwhere(cand != want_c)[:5].tolist())
            err = row_rel(logpj, want)
            print("pm_bsc_weighted_estep_f64 H=%d D=%d H'=%d %-6s row-relative error %.3e" % (H, D, Hp, layout, err))
            assert np.isfinite(logpj).all() and err <= RTOL, (H, D, layout, err)
        if binary:
            cand_m, logpj_m = _run_bsc(dev, m, P, b, g, xn2, Om, Wt, "odd", masked=True)
            assert np.array_equal(cand, cand_m)
            _bits(logpj, logpj_m, (H, D, Hp))


# ------------------------------------------------------------------------------------------- pm_mca_weighted_estep_f64
# (D, rho, signed): one D per dimensions-per-lane instantiation (DPL 1, 2, 4, 8, 16), each reaching the lane's LAST slab of 64
# dimensions, one D that fills it (256), D = 1024 and D = 1; the two special roots and a general one
MCA_SHAPES = [(40, 21.0, False), (100, 6.0, True), (200, 3.5, False), (500, 3.5, True), (1000, 21.0, False), (256, 6.0, True),
              (1024, 6.0, True), (1, 21.0, False)]


@pytest.mark.parametrize("D,rho,signed", MCA_SHAPES)
def test_mca_weighted_estep(dev, D, rho, signed):
    """[null ; H one-cause ; S multi-cause] log-joints and the two row log-sum-exps (beta = 0.8) against NumPy at 1e-11
    row-relative, padded lds / ldwn / ldx / ldo / ldl; with omega in {0, 1} the bits of pm_mca_masked_estep_f64."""
    from prosper_amd import _lib
    H, Hp, gam, N = 20, 5, 2, 9
    m = _mca_model(D, H, Hp, gam, signed)
    P = m._params({"T": 1.25}, 0.1, 0.9, rho)
    S = m.no_states
    K = 1 + H + S
    Wt, Wrho = _mca_weights(H, D, rho, signed, D)
    rng = np.random.RandomState(D + 1)
    cand = np.array([rng.permutation(H)[:Hp] for _ in range(N)], dtype=np.int32)
    SM = np.asarray(m.state_matrix) != 0
    masks = m._u16_dev(m._state_masks())
    Yfull = rng.uniform(-1 if signed else 0, 3, size=(N, D))

    def call(entry, eo, ops, layout):
        A, wn, xn2, X0 = ops
        ea, ewn = Emb(A, _ld(H, layout, 0), dev), Emb(wn, _ld(H, layout, 1), dev)
        en, ex = Emb(xn2, N, dev), Emb(X0, _ld(D, layout, 2), dev)
        ewr, ec = Emb(Wrho, D, dev), Emb(cand, Hp, dev)
        el = Emb(np.zeros((N, K)), _ld(K, layout, 4), dev, fill=False)
        e1, eb = Emb(np.zeros(N), N, dev, fill=False), Emb(np.zeros(N), N, dev, fill=False)
        _lib.call(entry, ea.ptr, ea.ld, ewn.ptr, ewn.ld, en.ptr, ex.ptr, ex.ld, eo.ptr, eo.ld, ewr.ptr, ec.ptr,
                  ctypes.c_void_p(masks.data_ptr()), S, ctypes.byref(P), N, H, D, Hp, el.ptr, el.ld, e1.ptr, eb.ptr, _stream())
        torch.cuda.synchronize()
        assert el.outside_untouched() and e1.outside_untouched() and eb.outside_untouched() and el.written(), (D, layout)
        assert _ok(ea, ewn, en, ex, eo, ewr, ec), (D, layout)
        return el.host(), e1.host()[0], eb.host()[0]

    for binary in (False, True):
        Om = _weights(N, D, D + 2, binary)
        X0 = np.where(Om != 0, Yfull, 0.0)
        ops = ((Om * X0) @ Wt.T, Om @ (Wt * Wt).T, (Om * X0 * X0).sum(axis=1), X0)
        A, wn, xn2, _ = ops
        want = np.empty((N, K))
        want[:, 0] = P.pre1 * xn2
        want[:, 1:1 + H] = P.pil_bar + P.pre1 * (wn - 2.0 * A + xn2[:, None])
        for n in range(N):
            for s, row in enumerate(SM):
                T = Wrho[cand[n, row]].sum(axis=0)
                wbar = np.sign(T) * np.abs(T) ** (1. / rho)
                want[n, 1 + H + s] = P.pil_bar * row.sum() + P.pre1 * (Om[n] * np.where(Om[n] != 0, wbar - X0[n], 0.0) ** 2).sum()
        for layout in (LAYOUTS if not binary else ["even"]):
            got, l1, lb = call("pm_mca_weighted_estep_f64", Emb(Om, _ld(D, layout, 3), dev), ops, layout)
            err = row_rel(got, want)
            print("pm_mca_weighted_estep_f64 D=%d rho=%g signed=%d %-6s row-relative error %.3e" % (D, rho, signed, layout, err))
            assert np.isfinite(got).all() and err <= RTOL, (D, rho, layout, err)
            np.testing.assert_allclose(l1, logsumexp(want, axis=1), rtol=RTOL)
            np.testing.assert_allclose(lb, logsumexp(P.beta * want, axis=1), rtol=RTOL)
        if binary:
            got_m, l1_m, lb_m = call("pm_mca_masked_estep_f64", emb_mask(Om.astype(np.uint8), _ld(D, "even", 3), dev), ops, "even")
            _bits(got, got_m, (D, "logpj"))
            _bits(l1, l1_m, (D, "lse1"))
            _bits(lb, lb_m, (D, "lseb"))
