"""The kernels of reconstruct(variance=True) (recon_var.hip) through the C ABI -- pm_recon_moments2_f64,
pm_recon_gsc_moments2_f64, pm_recon_var_finish_f64, pm_recon_mca_var_f64 -- on padded operands (the ``Emb`` harness of
tests/test_eval_kernels_gpu.py: pattern-filled guard rows and padding columns, inputs bit-unchanged) against the NumPy m2 / p /
V of tests/recon_var_reference.py, one case per branch of each kernel, and every PM_EINVAL / PM_ERANGE case on device
pointers (null pointers refused at N = 0 too).

Bounds.  m2 and p are sums of exp-weights times small table values: the modules' 1e-11 row-relative.  V: per row max_d
|V - V_ref| <= 4e-11 max_d E_ref[ybar_d^2] (RV.VTOL); where the operands are integers (finish kernel) equality."""
import ctypes

import numpy as np
import pytest
from scipy.special import logsumexp

import recon_reference as R
import recon_var_reference as RV
from test_eval_kernels_gpu import (LAYOUTS, RTOL, Emb, _ld, _mca_model, _mca_weights, _ok, _stream, _table_states, dev,  # noqa: F401
                                   ints, row_rel)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PM_EINVAL, PM_ERANGE = -1, -2


# ------------------------------------------------------------------------------------------------ pm_recon_moments2_f64
def _run_moments2(dev, X, a, off, cand, table, blocks, H, soff, moff, out_cols, layout, lse=None, with_p=True):
    from prosper_amd import _lib
    N, K = X.shape
    S = 0 if table is None else table.shape[0]
    Hp = 0 if table is None else table.shape[1]
    npair = Hp * (Hp - 1) // 2
    ex = Emb(X, _ld(K, layout, 0) if layout != "tight" else K + 5, dev)
    em = Emb(np.zeros((N, out_cols)), _ld(out_cols, layout, 1) if layout != "tight" else out_cols + 3, dev, fill=False)
    ep = Emb(np.zeros((N, npair)), _ld(npair, layout, 2) if layout != "tight" else npair + 1, dev, fill=False) \
        if (npair and with_p) else None
    eoff = Emb(off, K, dev) if off is not None else None
    elw = Emb(lse, N, dev) if lse is not None else None
    ec = Emb(np.asarray(cand, dtype=np.int32), Hp, dev) if S else None
    et = Emb(np.asarray(table, dtype=np.float64), Hp, dev) if S else None
    bv = (ctypes.c_double * 8)(*([float(v) for v in blocks] + [0.0] * (8 - len(blocks))))
    _lib.call("pm_recon_moments2_f64", ex.ptr, ex.ld, elw.ptr if elw else None, ctypes.c_double(a),
              eoff.ptr if eoff else None, ec.ptr if S else None, et.ptr if S else None, bv, N, H, Hp, K, soff, len(blocks), moff,
              S, em.ptr, em.ld, out_cols, ep.ptr if ep else None, ep.ld if ep else 1, _stream())
    torch.cuda.synchronize()
    assert em.ld > out_cols and ex.ld > K
    assert em.outside_untouched() and (ep is None or ep.outside_untouched()), "a padding column or a guard row was written"
    assert all(e.unchanged() for e in (ex, eoff, elw, ec, et) if e is not None)
    got = em.host()
    assert np.array_equal(got[:, H:], np.zeros((N, out_cols - H))), "columns [H, out_cols) are 0"
    want_m2, want_p = RV.moments2_from_lpj(X, a, cand, H, blocks, soff, moff, table, off=off)
    return got[:, :H], (ep.host() if ep else None), want_m2, want_p


def _check_mp(tag, got_m2, got_p, want_m2, want_p):
    e1 = row_rel(got_m2, want_m2)
    # p holds signed terms that cancel: relative to the row's largest second moment (the scale its error reaches V with)
    e2 = 0.0 if got_p is None else float((np.abs(got_p - want_p).max(axis=1) / np.abs(want_m2).max(axis=1)).max())
    print("pm_recon_moments2_f64 %-34s m2 %.3e  p %.3e (bound %.1e)" % (tag, e1, e2, RTOL))
    assert e1 <= RTOL and e2 <= RTOL, (tag, e1, e2)


@pytest.mark.parametrize("layout", ["tight", "even", "odd"])
def test_recon_moments2(dev, layout):
    rng = np.random.RandomState(10 + len(layout))
    N = 11
    # BSC layout, H = 70 > 64 (the lane-strided loop), H' = 12: 66 pairs, a lane owns two; lse formed and given
    H, Hp = 70, 12
    tab = _table_states(Hp, 2, [1.0], rng)
    X = 3.0 * rng.normal(size=(N, 1 + H + len(tab)))
    cand = np.array([np.sort(rng.permutation(H)[:Hp]) for _ in range(N)])
    for lse in (None, logsumexp(X, axis=1)):
        _check_mp("bsc H'=12 %s lse %s" % (layout, "formed" if lse is None else "given"),
                  *_run_moments2(dev, X, 1.0, None, cand, tab, (1.0,), H, 1, 1 + H, 72, layout, lse=lse))
    # DSC layout with 8 latent values (7 blocks), H = 130 (three trips of the H loop), H' = 16: 120 pairs, the limit
    H, vals = 130, (-3., -2., -1., 1., 2., 3., 4.)
    tab = _table_states(16, 2, vals, rng)
    X = 3.0 * rng.normal(size=(N, 1 + 7 * H + len(tab)))
    cand = np.array([np.sort(rng.permutation(H)[:16]) for _ in range(N)])
    _check_mp("dsc8 H=130 H'=16 " + layout, *_run_moments2(dev, X, 1.0, None, cand, tab, vals, H, 1, 1 + 7 * H, 136, layout))
    # DSC with 2 non-zero values, H = 65 (one lane takes a second latent), H' = 2: one pair
    H, vals = 65, (-1., 2.)
    tab = np.array([[a_, b_] for a_ in vals for b_ in vals])
    X = 3.0 * rng.normal(size=(N, 1 + 2 * H + len(tab)))
    cand = np.array([np.sort(rng.permutation(H)[:2]) for _ in range(N)])
    _check_mp("dsc3 H=65 H'=2 " + layout, *_run_moments2(dev, X, 1.0, None, cand, tab, vals, H, 1, 1 + 2 * H, 72, layout))
    # H' = 1: a table, no pairs, p = NULL
    tab = np.array([[-1.0], [1.0], [2.0]])
    X = 3.0 * rng.normal(size=(N, 1 + H + 3))
    cand = rng.randint(0, H, size=(N, 1))
    g = _run_moments2(dev, X, 1.0, None, cand, tab, (1.0,), H, 1, 1 + H, 65, layout)
    assert g[1] is None
    _check_mp("H'=1 " + layout, *g)
    # TSC layout: table states only, 375 > 256 of them (a second LDS chunk), rows whose candidates repeat a latent
    H, Hp = 70, 10
    tab = _table_states(Hp, 4, [-1.0, 1.0], rng)
    assert len(tab) == 375
    X = 3.0 * rng.normal(size=(N, len(tab)))
    cand = np.array([rng.permutation(H)[:Hp] for _ in range(N)])
    cand[2, 3] = cand[2, 0]
    cand[5, 4] = cand[5, 1] = cand[5, 2]
    cand[7, :] = 69
    _check_mp("tsc S=375 repeated " + layout, *_run_moments2(dev, X, 1.0, None, cand, tab, (), H, 0, 0, 72, layout))
    # mixture use: S = 0, one block of value 1, a != 1 with a column offset: m2 is the row softmax
    H = 21
    X, off = 3.0 * rng.normal(size=(N, H)), rng.normal(size=H)
    got, _, want, _ = _run_moments2(dev, X, 0.7, off, None, None, (1.0,), H, 0, 0, 24, layout)
    assert row_rel(got, R.softmax_rows(0.7 * X + off[None, :])) <= RTOL and row_rel(got, want) <= RTOL


def test_recon_moments2_second_trip_nan_row_and_bits(dev):
    """N = 8269 > 2048 workgroups of four rows: the rows past 8192 are a wavefront's second trip.  A NaN row is NaN in m2 and p
    and nowhere else; the two libraries and a second call give the same bits."""
    from prosper_amd import _lib
    rng = np.random.RandomState(3)
    N, H, Hp = 8269, 6, 4
    tab = _table_states(Hp, 3, [1.0], rng)
    K = 1 + H + len(tab)
    X = 3.0 * rng.normal(size=(N, K))
    X[8200, 2] = np.nan
    cand = np.array([np.sort(rng.permutation(H)[:Hp]) for _ in range(N)], dtype=np.int32)
    want_m2, want_p = RV.moments2_from_lpj(X, 1.0, cand, H, (1.0,), 1, 1 + H, tab)
    ex, ec, et = Emb(X, K + 1, dev), Emb(cand, Hp, dev), Emb(tab, Hp, dev)
    one = (ctypes.c_double * 8)(1.0)
    outs = []
    for det in (False, True, False):
        em, ep = Emb(np.zeros((N, 8)), 9, dev, fill=False), Emb(np.zeros((N, 6)), 7, dev, fill=False)
        _lib.call("pm_recon_moments2_f64", ex.ptr, ex.ld, None, ctypes.c_double(1.0), None, ec.ptr, et.ptr, one, N, H, Hp, K, 1, 1,
                  1 + H, len(tab), em.ptr, em.ld, 8, ep.ptr, ep.ld, _stream(), det=det)
        torch.cuda.synchronize()
        assert em.outside_untouched() and ep.outside_untouched() and em.written() and ep.written()
        outs.append((em.host(), ep.host()))
    m2, p = outs[0]
    assert np.isnan(m2[8200, :H]).all() and np.isnan(p[8200]).all()
    keep = np.arange(N) != 8200
    assert np.isfinite(m2[keep]).all() and np.isfinite(p[keep]).all()
    _check_mp("second trip", m2[keep][:, :H], p[keep], want_m2[keep], want_p[keep])
    for o in outs[1:]:
        assert np.array_equal(o[0].view(np.uint64), m2.view(np.uint64)) and np.array_equal(o[1].view(np.uint64), p.view(np.uint64))


# ---------------------------------------------------------------------------------------------- pm_recon_var_finish_f64
@pytest.mark.parametrize("D", [1, 63, 64, 65, 1100])
def test_recon_var_finish(dev, D):
    """Integer operands: every term is an integer far below 2^53, so V equals NumPy's bit for bit -- with H' = 5 pairs and mu,
    with p = NULL (cand and Wt NULL too), at H' = 16 (120 pairs), leading dimensions larger than D; a negative value is
    returned as 0, a NaN stays NaN in its row alone; N = 8269 at D = 1 for the second trip."""
    from prosper_amd import _lib
    H = 40
    for Hp, with_mu, N in ((5, True, 9), (16, False, 6), (0, False, 9)) + (((3, True, 8269),) if D == 1 else ()):
        rng = np.random.RandomState(D + Hp)
        npair = Hp * (Hp - 1) // 2
        W = ints(D, H, D + 1, -4, 4)
        V0 = ints(N, D, D + 2, 0, 50)
        Yh = ints(N, D, D + 3, -5, 5)
        mu = ints(1, D, D + 4, -3, 3)[0] if with_mu else None
        p = ints(N, max(npair, 1), D + 5, -3, 3)[:, :npair]
        cand = np.array([rng.permutation(H)[:Hp] for _ in range(N)], dtype=np.int32).reshape(N, Hp)
        if Hp >= 3:
            cand[1, 2] = cand[1, 0]                                          # a repeated candidate: the pair counts W^2
        if N > 4:
            Yh[4, 0] = np.nan
        want = RV.finish(None, p if npair else None, cand, W, Yh, mu, V0=V0)
        assert (want == 0).any() or D == 1                                    # (the clamp is reached)
        for layout in ["tight", "odd", "mix_a"] if N < 100 else ["odd"]:
            ev = Emb(V0, _ld(D, layout, 1) if layout != "tight" else D + 3, dev)
            ey = Emb(Yh, _ld(D, layout, 2) if layout != "tight" else D + 1, dev)
            emu = Emb(mu, D, dev) if with_mu else None
            ep = Emb(p, _ld(npair, layout, 2) if layout != "tight" else npair + 2, dev) if npair else None
            ec = Emb(cand, Hp, dev) if npair else None
            ew = Emb(np.ascontiguousarray(W.T), _ld(D, layout, 0) if layout != "tight" else D + 5, dev) if npair else None
            _lib.call("pm_recon_var_finish_f64", ev.ptr, ev.ld, ey.ptr, ey.ld, emu.ptr if emu else None, ep.ptr if ep else None,
                      ep.ld if ep else 1, ec.ptr if ec else None, ew.ptr if ew else None, ew.ld if ew else D, N, H, D, Hp,
                      _stream())
            torch.cuda.synchronize()
            got = ev.host()
            assert ev.ld > D and ev.outside_untouched(), (D, Hp, layout)
            assert all(e.unchanged() for e in (ey, emu, ep, ec, ew) if e is not None)
            if N > 4:
                assert np.isnan(got[4, 0]) and np.isfinite(np.delete(got.ravel(), 4 * D)).all()
            assert np.array_equal(np.nan_to_num(got, nan=-1.0), np.nan_to_num(want, nan=-1.0)), (D, Hp, layout)
            assert (np.nan_to_num(got) >= 0).all()


# ------------------------------------------------------------------------------------------------- pm_recon_mca_var_f64
@pytest.mark.parametrize("D,rho,signed", [(1, 21.0, False), (70, 6.0, True), (200, 3.5, False), (500, 21.0, False),
                                          (1024, 6.0, True), (1024, 21.0, False)])
def test_recon_mca_var(dev, D, rho, signed):
    """V += sum_s q_s Wbar(s)^2 into a NON-ZERO V with a padded row, the row log-sum-exp given and formed by the kernel: V0
    plus NumPy's increment at 1e-11 row-relative (every term is positive)."""
    from prosper_amd import _lib
    H, Hp, gam, N = 20, 5, 2, 9
    m = _mca_model(D, H, Hp, gam, signed)
    S = m.no_states
    K = 1 + H + S
    _, Wrho = _mca_weights(H, D, rho, signed, D + 7)
    rng = np.random.RandomState(D + 3)
    lp = 2.0 * rng.normal(size=(N, K))
    lse = logsumexp(lp, axis=1)
    cand = np.array([rng.permutation(H)[:Hp] for _ in range(N)], dtype=np.int32)
    V0 = rng.uniform(size=(N, D))
    inc = np.zeros((N, D))
    for n in range(N):
        for s, row in enumerate(np.asarray(m.state_matrix) != 0):
            T = Wrho[cand[n, row]].sum(axis=0)
            wbar = np.sign(T) * np.abs(T) ** (1. / rho) if signed else T ** (1. / rho)
            inc[n] += np.exp(lp[n, 1 + H + s] - lse[n]) * wbar * wbar
    assert inc.max() > 0.1
    want = V0 + inc
    masks = m._u16_dev(m._state_masks())
    for layout in ("tight", "odd", "mix_b"):
        for given in (False, True):
            el, els = Emb(lp, _ld(K, layout, 0), dev), Emb(lse, N, dev)
            ec, ewr = Emb(cand, Hp, dev), Emb(Wrho, D, dev)
            ev = Emb(V0, _ld(D, layout, 1) if layout != "tight" or given else D + 3, dev)
            _lib.call("pm_recon_mca_var_f64", el.ptr, el.ld, els.ptr if given else None, ec.ptr,
                      ctypes.c_void_p(masks.data_ptr()), ewr.ptr, ctypes.c_double(1. / rho), int(signed), N, H, D, Hp, S, ev.ptr,
                      ev.ld, _stream())
            torch.cuda.synchronize()
            err = row_rel(ev.host(), want)
            print("pm_recon_mca_var_f64 D=%d rho=%g signed=%d %-6s lse %s row-relative error %.3e" % (
                D, rho, signed, layout, "given" if given else "formed", err))
            assert err <= RTOL, (D, rho, layout, given, err)
            assert ev.outside_untouched() and _ok(el, els, ec, ewr), (D, layout, given)


# ------------------------------------------------------------------------------------------ pm_recon_gsc_moments2_f64
def test_recon_gsc_moments2(dev):
    """Synthetic operands (the entry only combines them): against the same arithmetic in NumPy -- weights exp(beta lp) floored
    at DBL_MIN but for the null state, Z + DBL_MIN, the singletons' kappa^2 + 1 / lambda from the tables, the candidate block's
    diagonal and the mean of its two triangles; H = 70 > 64, H' = 12 (66 pairs); blocks = NULL (no multi-cause states); a
    row whose weights all underflow (the floor) and a NaN row."""
    from prosper_amd import _lib
    rng = np.random.RandomState(17)
    N, H, Hp, S, beta = 13, 70, 12, 9, 0.5
    HH, npair = Hp * Hp, Hp * (Hp - 1) // 2
    tiny = np.finfo(np.float64).tiny
    lp = 4.0 * rng.normal(size=(N, 1 + H + S))
    lp[3] = -4000.0 + rng.normal(size=1 + H + S)
    sc = rng.normal(size=(N, H))
    sc[6, 5] = np.nan
    lp[6, 1:] = np.nan
    tables = rng.uniform(0.5, 1.5, size=(8, H))
    blk = rng.uniform(0.1, 2.0, size=(N, 2 * HH + 2 * Hp + 1))
    blk[3] *= 1e-300
    cand = np.array([np.sort(rng.permutation(H)[:Hp]) for _ in range(N)], dtype=np.int32)
    gm, kl, ilam, mu = tables[2], tables[4], tables[5], tables[6]
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.where(beta * lp[:, 1:1 + H] >= -708.3964185322641, np.maximum(np.exp(beta * lp[:, 1:1 + H]), tiny), tiny)
        kap = (sc - gm) * kl + mu
    pairs = [(i, j) for i in range(Hp) for j in range(i + 1, Hp)]
    for with_blocks in (True, False):
        Z = np.exp(beta * lp[:, 0]) + w.sum(axis=1) + (blk[:, -1] if with_blocks else 0.0)
        nf = 1.0 / (Z + tiny)
        want_m2 = w * (kap * kap + ilam) * nf[:, None]
        want_p = np.zeros((N, npair))
        if with_blocks:
            szsz = blk[:, HH:2 * HH].reshape(N, Hp, Hp)
            for i in range(Hp):
                want_m2[np.arange(N), cand[:, i]] += szsz[:, i, i] * nf
            want_p = np.stack([0.5 * (szsz[:, i, j] + szsz[:, j, i]) * nf for i, j in pairs], axis=1)
        el, eb, es, et, ec = Emb(lp, lp.shape[1] + 3, dev), Emb(blk, blk.shape[1] + 2, dev), Emb(sc, H + 1, dev), \
            Emb(tables.reshape(1, -1), 8 * H, dev), Emb(cand, Hp, dev)
        em, ep = Emb(np.zeros((N, 72)), 75, dev, fill=False), Emb(np.zeros((N, npair)), npair + 1, dev, fill=False)
        _lib.call("pm_recon_gsc_moments2_f64", el.ptr, el.ld, eb.ptr if with_blocks else None, eb.ld, es.ptr, es.ld, et.ptr,
                  ec.ptr, ctypes.c_double(beta), N, H, Hp, S, em.ptr, em.ld, 72, ep.ptr, ep.ld, _stream())
        torch.cuda.synchronize()
        assert em.outside_untouched() and ep.outside_untouched() and _ok(el, eb, es, et, ec)
        m2, p = em.host(), ep.host()
        assert np.array_equal(m2[:, H:], np.zeros((N, 2)))
        assert np.isnan(m2[6, 5]) and np.isfinite(np.delete(m2, 6, axis=0)).all() and np.isfinite(np.delete(p, 6, axis=0)).all()
        keep = np.arange(N) != 6
        e1 = row_rel(m2[keep][:, :H], want_m2[keep])
        e2 = row_rel(p[keep], want_p[keep]) if with_blocks else float(np.abs(p[keep]).max())
        print("pm_recon_gsc_moments2_f64 blocks %d: m2 %.3e  p %.3e" % (with_blocks, e1, e2))
        assert e1 <= RTOL and e2 <= RTOL


# ------------------------------------------------------------------------------------------------------ argument checks
def test_argument_checks_on_device_pointers(dev):
    """Each PM_EINVAL and PM_ERANGE case with real device buffers behind the other arguments: no output is written."""
    from prosper_amd import _lib
    lib = _lib.load()
    big = Emb(np.zeros((8, 700)), 700, dev, fill=False)
    ci = Emb(np.zeros((8, 17), dtype=np.int32), 17, dev)
    p = big.ptr
    one = (ctypes.c_double * 8)(1.0)
    st = _stream()

    def mom(logpj=p, ld=10, lse=None, a=1.0, off=None, cand=ci.ptr, vals=p, bv=one, N=4, H=4, Hp=3, K=9, soff=1, nblk=1, moff=5,
            S=4, m2=p, ldm=8, cols=8, pp=p, ldp=3):
        return lib.pm_recon_moments2_f64(logpj, ld, lse, a, off, cand, vals, bv, N, H, Hp, K, soff, nblk, moff, S, m2, ldm, cols,
                                         pp, ldp, st)
    for N in (4, 0):
        for k in ("logpj", "cand", "vals", "bv", "m2", "pp"):
            assert mom(N=N, **{k: None}) == PM_EINVAL, (k, N)
    assert mom(N=-1) == PM_EINVAL and mom(ld=8) == PM_EINVAL and mom(ldm=7) == PM_EINVAL and mom(ldp=2) == PM_EINVAL
    assert mom(moff=6) == PM_EINVAL and mom(lse=p, a=0.5) == PM_EINVAL and mom(Hp=0) == PM_EINVAL
    assert mom(Hp=17, ldp=200) == PM_ERANGE and mom(nblk=9, K=200, ld=200) == PM_ERANGE

    def gsc(lp=p, ldl=12, blk=p, ldb=25, sc=p, lds=4, tab=p, cand=ci.ptr, beta=0.5, N=4, H=4, Hp=3, S=4, m2=p, ldm=8, cols=8, pp=p,
            ldp=3):
        return lib.pm_recon_gsc_moments2_f64(lp, ldl, blk, ldb, sc, lds, tab, cand, beta, N, H, Hp, S, m2, ldm, cols, pp, ldp, st)
    for N in (4, 0):
        for k in ("lp", "sc", "tab", "cand", "m2", "pp"):
            assert gsc(N=N, **{k: None}) == PM_EINVAL, (k, N)
    assert gsc(N=-1) == PM_EINVAL and gsc(ldl=8) == PM_EINVAL and gsc(ldb=24) == PM_EINVAL and gsc(lds=3) == PM_EINVAL
    assert gsc(ldm=7) == PM_EINVAL and gsc(ldp=2) == PM_EINVAL and gsc(beta=-1.0) == PM_EINVAL
    assert gsc(Hp=17, ldb=700, ldp=200) == PM_ERANGE

    def fin(V=p, ldv=10, Y=p, ldy=10, mu=None, pp=p, ldp=3, cand=ci.ptr, Wt=p, ldw=10, N=4, H=4, D=10, Hp=3):
        return lib.pm_recon_var_finish_f64(V, ldv, Y, ldy, mu, pp, ldp, cand, Wt, ldw, N, H, D, Hp, st)
    for N in (4, 0):
        for k in ("V", "Y", "cand", "Wt"):
            assert fin(N=N, **{k: None}) == PM_EINVAL, (k, N)
    assert fin(N=-1) == PM_EINVAL and fin(D=0) == PM_EINVAL and fin(ldv=9) == PM_EINVAL and fin(ldy=9) == PM_EINVAL
    assert fin(ldw=9) == PM_EINVAL and fin(ldp=2) == PM_EINVAL and fin(Hp=17, ldp=200) == PM_ERANGE

    def mca(logpj=p, ld=100, cand=ci.ptr, masks=p, Wrho=p, inv_rho=1 / 21., N=4, H=4, D=10, Hp=2, S=1, V=p, ldv=None):
        return lib.pm_recon_mca_var_f64(logpj, ld, None, cand, masks, Wrho, inv_rho, 0, N, H, D, Hp, S, V,
                                        D if ldv is None else ldv, st)
    for N in (4, 0):
        for k in ("logpj", "cand", "masks", "Wrho", "V"):
            assert mca(N=N, **{k: None}) == PM_EINVAL, (k, N)
    assert mca(N=-1) == PM_EINVAL and mca(ld=5) == PM_EINVAL and mca(ldv=9) == PM_EINVAL and mca(inv_rho=0.0) == PM_EINVAL
    assert mca(D=1025, ldv=1025) == PM_ERANGE and mca(Hp=17) == PM_ERANGE
    torch.cuda.synchronize()
    assert big.unchanged() and ci.unchanged()
    assert mom(N=0) == 0 and gsc(N=0) == 0 and fin(N=0) == 0 and mca(N=0) == 0 and mca(S=0) == 0
    torch.cuda.synchronize()
    assert big.unchanged()
