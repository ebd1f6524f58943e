"""reconstruct(..., exact=True) on the device: against NumPy enumeration of every state, against the project's own
truncated path at H' = gamma = H, against a closed form past NumPy's reach, bit for bit across calls, builds, row orders,
shards, row blocks and image chunkings, with a training run undisturbed, at the limits and refusals.
NumPy references: tests/recon_reference.py; problems per model: tests/test_reconstruct_gpu.py.

Tolerance: the project's bound for reconstruct against enumeration, |delta| / max_d |yhat_nd| <= 1e-11
per row (recon_reference.row_rel_err); against the truncated path 2e-11, each side being within 1e-11 of the truth.  The
measured deviations on the MI355X are recorded in DESIGN 4.18, which also names the kernel branch every shape reaches."""
import time

import numpy as np
import pytest

import patches_reference as P
import recon_reference as R
from test_reconstruct_gpu import _mixture, _problem, _tsc_distinct

pytestmark = pytest.mark.gpu

RTOL = 1e-11


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def _check(tag, got, want, rtol=RTOL):
    err = R.row_rel_err(got, want)
    print("reconstruct exact %-34s row-relative error %.3e (bound %.1e)" % (tag, err, rtol))
    assert got.shape == want.shape and got.dtype == np.float64
    assert err <= rtol, (tag, err)


def _bits(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype == np.float64, what
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), what


def _entries(m):
    """The model's launch hook, wrapped to keep the names of the entry points that ran."""
    calls = []
    orig = m._call
    m._call = lambda label, entry, *args: (calls.append(entry), orig(label, entry, *args))[1]
    return calls


def _dsc(rng, D, H, N, states, pi, Hp=3, g=2):
    from prosper_amd.em.camodels.dsc_et import DSC_ET
    states, pi = np.asarray(states, dtype=np.float64), np.asarray(pi, dtype=np.float64)
    W, sigma = rng.normal(size=(D, H)), 0.9
    Y = states[rng.choice(len(states), p=pi, size=(N, H))] @ W.T + sigma * rng.normal(size=(N, D))
    with np.errstate(divide="ignore"):
        lp = np.log(pi)
    return (DSC_ET(D, H, Hp, g, states=states), {"W": W, "pi": pi, "sigma": sigma}, Y,
            lambda Y: R.enum_linear(Y, W, sigma, states, lp))


# ------------------------------------------------------------------------------------------ 1: against NumPy enumeration
# (name, D, H, N): the branch of recon_exact.hip each shape reaches is listed in DESIGN 4.18
ENUM = [("bsc", 20, 6, 37), ("bsc_mu", 20, 6, 37), ("bsc", 20, 13, 67), ("tsc", 20, 8, 37),
        ("mca", 20, 6, 37), ("mmca", 20, 6, 37), ("mca", 70, 10, 18), ("mmca", 70, 10, 18), ("mca", 1, 4, 37),
        ("mca", 1024, 4, 3),
        ("gsc_scalar", 20, 5, 37), ("gsc_diagonal", 20, 5, 37), ("gsc_full", 20, 5, 37), ("gsc_scalar", 20, 10, 70)]


@pytest.mark.parametrize("name,D,H,N", ENUM)
def test_against_enumeration(dev, name, D, H, N):
    m, p, Y, _, enum = _problem(name, np.random.RandomState(7 * D + H), D, H, N, min(H, 3), 2)
    p_in = {k: np.array(v, copy=True) for k, v in p.items()}
    hp = (m.Hprime, m.gamma)
    calls = _entries(m)
    got = m.reconstruct(p, {"y": Y}, exact=True)
    for k in p_in:
        np.testing.assert_array_equal(p[k], p_in[k])
    assert set(p) == set(p_in) and (m.Hprime, m.gamma) == hp
    kind = "gsc" if name.startswith("gsc") else ("mca" if name in ("mca", "mmca") else "lin")
    assert "pm_recon_exact_%s_f64" % kind in calls, calls
    assert not [c for c in calls if "estep" in c or "select" in c or c == "pm_recon_expect_f64"], calls
    _check("%s D=%d H=%d N=%d" % (name, D, H, N), got, enum(Y))


def test_dsc_with_a_value_of_zero_prior(dev):
    m, p, Y, enum = _dsc(np.random.RandomState(41), 20, 6, 37, [0., 1., 2., 3.], [0.6, 0.25, 0.0, 0.15])
    _check("dsc 4 values, one of zero prior", m.reconstruct(p, {"y": Y}, exact=True), enum(Y))


def test_dsc_with_five_values(dev):
    m, p, Y, enum = _dsc(np.random.RandomState(42), 20, 5, 37, [-2., -1., 0., 1., 2.], [0.1, 0.15, 0.5, 0.15, 0.1])
    _check("dsc 5 values", m.reconstruct(p, {"y": Y}, exact=True), enum(Y))


# --------------------------------------------------------------------------- 2: against the project's own truncated path
def _trio(name, D, H, N, seed):
    """Three models of one problem, built with (H', gamma) = (3, 2), (5, 3) and (H, H); parameters and data of the first."""
    if name.startswith("dsc"):
        # the truncated side holds its state table in LDS (S H' bytes within 150 KiB, pm_dsc_plan): at H' = gamma = H = 10
        # that admits two latent values (2^10 states), and three values up to H = 8 (3^8)
        states, pi = ([0., 1.5], [0.75, 0.25]) if name == "dsc2" else ([-1., 0., 1.], [0.15, 0.7, 0.15])
        mk = lambda hp, g, n: _dsc(np.random.RandomState(seed), D, H, n, states, pi, hp, g)
        small, p, Y, _ = mk(3, 2, N)
        return small, mk(5, 3, 1)[0], mk(H, H, 1)[0], p, Y
    small, p, Y, _, _ = _problem(name, np.random.RandomState(seed), D, H, N, 3, 2)
    return (small, _problem(name, np.random.RandomState(0), D, H, 1, 5, 3)[0],
            _problem(name, np.random.RandomState(0), D, H, 1, H, H)[0], p, Y)


@pytest.mark.parametrize("name,D,H", [("bsc", 20, 10), ("dsc2", 20, 10), ("dsc3", 20, 8), ("mca", 20, 10), ("mmca", 20, 10),
                                      ("tsc", 12, 6), ("gsc_scalar", 20, 6)])
def test_against_the_truncated_path_at_full_width(dev, name, D, H):
    """exact=True of a model built with (H', gamma) = (3, 2) against reconstruct() of a second model with H' = gamma = H; and
    the same bits from a model built with (5, 3)."""
    N = 100 if name != "tsc" else 300
    small, other, full, p, Y = _trio(name, D, H, N, 1 if name == "tsc" else 50 + H + len(name))
    got = small.reconstruct(p, {"y": Y}, exact=True)
    _bits(other.reconstruct(p, {"y": Y}, exact=True), got, "%s: (3, 2) against (5, 3)" % name)
    want = full.reconstruct(p, {"y": Y})
    keep = np.ones(N, dtype=bool)
    if name == "tsc":              # rows whose candidates repeat a latent hold pseudo-states on the truncated side
        keep = _tsc_distinct(p, Y, D, H)
        assert keep.sum() >= N // 2, keep.sum()
    _check("%s H=%d against H'=gamma=H" % (name, H), got[keep], want[keep], rtol=2e-11)


# --------------------------------------------------------------------------------- 3: closed form past NumPy's reach
def _closed_form(D, N, seed):
    """BSC with W = c I (D = H) and mu: the posterior factorises over the latents."""
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    rng = np.random.RandomState(seed)
    c, pi, sigma = 1.7, 0.3, 0.9
    mu = rng.normal(size=D)
    S = rng.uniform(size=(N, D)) < pi
    Y = mu + c * S + sigma * rng.normal(size=(N, D))
    es = 1.0 / (1.0 + np.exp(-(np.log(pi / (1 - pi)) + (c * (Y - mu) - 0.5 * c * c) / sigma ** 2)))
    return BSC_ET(D, D, 3, 2), {"W": c * np.eye(D), "pi": pi, "sigma": sigma, "mu": mu}, Y, mu + c * es


def test_closed_form_2_to_the_24_states(dev):
    m, p, Y, want = _closed_form(24, 3, 5)
    _check("bsc W = c I, H = 24", m.reconstruct(p, {"y": Y}, exact=True), want)


def test_closed_form_2_to_the_32_states(dev):
    import torch
    m, p, Y, want = _closed_form(32, 1, 6)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = m.reconstruct(p, {"y": Y}, exact=True)
    print("reconstruct exact: 2^32 states, one row: %.2f s" % (time.perf_counter() - t0))
    _check("bsc W = c I, H = 32", got, want)


# --------------------------------------------------------------------------------------------------------------- 4: bits
@pytest.mark.parametrize("name,H", [("bsc", 6), ("mca", 6), ("gsc_scalar", 5), ("bsc_mu", 13), ("tsc", 8), ("mmca", 10)])
def test_bits_across_calls_builds_row_order_and_shards(dev, name, H):
    rng = np.random.RandomState(23)
    m, p, Y, _, _ = _problem(name, rng, 20, H, 67, 3, 2)
    a = m.reconstruct(p, {"y": Y}, exact=True)
    assert np.isfinite(a).all()
    _bits(m.reconstruct(p, {"y": Y}, exact=True), a, "second call")
    m.deterministic = True
    _bits(m.reconstruct(p, {"y": Y}, exact=True), a, "the deterministic library")
    m.deterministic = False
    perm = rng.permutation(67)
    _bits(m.reconstruct(p, {"y": Y[perm]}, exact=True), a[perm], "row permutation")
    _bits(m.reconstruct(p, {"y": Y[10:30]}, exact=True), a[10:30], "shard")
    _bits(m.reconstruct(p, {"y": Y[29:30]}, exact=True), a[29:30], "one row")


@pytest.mark.parametrize("name", ["bsc", "mca"])
def test_bits_inside_many_row_blocks(dev, name):
    """The same 67 rows inside N = 8269: every row block of the host walk but the first is a second trip."""
    rng = np.random.RandomState(29)
    m, p, Y, _, _ = _problem(name, rng, 20, 6, 8269, 3, 2)
    at = 5000 + 17
    a = m.reconstruct(p, {"y": Y[at:at + 67]}, exact=True)
    big = m.reconstruct(p, {"y": Y}, exact=True)
    assert big.shape == (8269, 20) and np.isfinite(big).all()
    _bits(big[at:at + 67], a, "%s: rows of a shard inside 8269" % name)
    _bits(big[-13:], m.reconstruct(p, {"y": Y[-13:]}, exact=True), "the ragged last block")


@pytest.mark.parametrize("name", ["bsc", "mca"])
def test_image_bits_do_not_depend_on_the_chunking(dev, name):
    rng = np.random.RandomState(31)
    m, p, _, _, _ = _problem(name, rng, 16, 6, 1, 3, 2)
    img = rng.normal(size=(19, 23)) + 1.0
    stride = 2
    nc = len(P.starts(23, 4, stride))
    whole = m.reconstruct_image(p, img, stride=stride, exact=True)
    for chunk in (nc, 3 * nc + 1):
        _bits(m.reconstruct_image(p, img, stride=stride, chunk=chunk, exact=True), whole, "chunk %d" % chunk)
    rows = m.reconstruct(p, {"y": P.extract(img, (4, 4), stride)}, exact=True)
    _bits(whole, P.average(rows, img.shape, (4, 4), stride), "the NumPy overlap average of the patches' rows")
    assert np.abs(whole - m.reconstruct_image(p, img, stride=stride)).max() > 0      # (not the truncated path's result)


@pytest.mark.parametrize("name,H", [("bsc", 6), ("tsc", 8), ("mca", 6), ("mca", 10), ("gsc_full", 5), ("gsc_scalar", 10)])
def test_nan_row_and_empty(dev, name, H):
    m, p, Y, _, _ = _problem(name, np.random.RandomState(11), 20, H, 70, 3, 2)
    clean_rows = m.reconstruct(p, {"y": np.delete(Y, 66, axis=0)}, exact=True)
    Y = Y.copy()
    Y[66, 2] = np.nan
    rows = m.reconstruct(p, {"y": Y}, exact=True)
    assert np.isnan(rows[66]).all() and np.isfinite(np.delete(rows, 66, axis=0)).all()
    _bits(np.delete(rows, 66, axis=0), clean_rows, "the other rows")
    calls = _entries(m)
    empty = m.reconstruct(p, {"y": np.zeros((0, 20))}, exact=True)
    assert empty.shape == (0, 20) and empty.dtype == np.float64 and not calls
    assert m.reconstruct(p, {"y": np.zeros((0, 20))}, device=True, exact=True).shape == (0, 20)


# -------------------------------------------------------------------------------------------- 5: training undisturbed
def _train(m, params, Y, Yh, steps, interleave):
    from prosper_amd.em.annealing import LinearAnnealing
    a = LinearAnnealing(steps)
    a["T"] = [(0, 2.), (.7, 1.)]
    a["Ncut_factor"] = [(0, 0.), (2. / 3, 1.)]
    a["anneal_prior"] = False
    a.as_dict = lambda: {k: a[k] for k in ("T", "Ncut_factor")}
    out = []
    for _ in range(steps):
        params = m.step(a, params, {"y": Y})
        out.append({k: np.array(v, copy=True) for k, v in params.items()})
        if interleave:
            hp = (m.Hprime, m.gamma)
            calls = _entries(m)
            try:
                rec = m.reconstruct({k: np.array(v, copy=True) for k, v in params.items()}, {"y": Yh}, exact=True)
            finally:
                del m._call
            assert rec.shape == Yh.shape and np.isfinite(rec).all() and (m.Hprime, m.gamma) == hp
            assert "pm_recon_exact_lin_f64" in calls, calls
            assert set(calls) <= {"pm_row_sqnorm_f64", "pm_recon_exact_lin_f64", "pm_gemm_nt_rows_f64"}, calls
        a.next()
    return out


def test_training_undisturbed(dev):
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    rng = np.random.RandomState(14)
    D, H, N = 24, 12, 2000
    p = {"W": rng.normal(size=(D, H)), "pi": 2.0 / H, "sigma": 1.2}
    Y = (rng.uniform(size=(N + 300, H)) < 2.0 / H) @ p["W"].T + rng.normal(size=(N + 300, D))

    def det():
        m = BSC_ET(D, H, 6, 3)
        m.deterministic = True
        return m
    ref = _train(det(), dict(p), Y[:N], Y[N:], 5, False)
    got = _train(det(), dict(p), Y[:N], Y[N:], 5, True)
    for pa, pb in zip(ref, got):
        for k in pa:
            np.testing.assert_array_equal(pa[k], pb[k], err_msg=k)


# ----------------------------------------------------------------------------------------------- 6: limits and refusals
@pytest.mark.parametrize("name,H", [("bsc", 33), ("gsc_scalar", 17)])
def test_past_the_state_bound_raises_before_any_launch(dev, name, H):
    from prosper_amd import _lib
    m, p, Y, _, _ = _problem(name, np.random.RandomState(3), 20, H, 5, 3, 2)
    calls = _entries(m)
    with pytest.raises(_lib.HipError):
        m.reconstruct(p, {"y": Y}, exact=True)
    assert not calls, calls


def test_mca_past_the_dimension_bound_raises(dev):
    from prosper_amd import _lib
    m, p, Y, _, _ = _problem("mca", np.random.RandomState(3), 1025, 4, 2, 3, 2)
    calls = _entries(m)
    with pytest.raises(_lib.HipError):
        m.reconstruct(p, {"y": Y}, exact=True)
    assert not calls, calls


@pytest.mark.parametrize("name", ["bsc", "mca", "tsc"])
def test_a_mask_with_exact_raises_before_any_launch(dev, name):
    m, p, Y, _, _ = _problem(name, np.random.RandomState(3), 20, 6, 9, 3, 2)
    calls = _entries(m)
    with pytest.raises(NotImplementedError, match="exact" if name != "tsc" else None):
        m.reconstruct(p, {"y": Y, "mask": np.ones(Y.shape, dtype=bool)}, exact=True)
    with pytest.raises(NotImplementedError, match="exact" if name != "tsc" else None):
        m.reconstruct_image(p, np.zeros((12, 12)), patch=(4, 5), mask=np.ones((12, 12), dtype=bool), exact=True)
    assert not calls, calls


@pytest.mark.parametrize("kind", ["mog_diagonal", "mog_full", "mop", "mop_A"])
def test_mixtures_return_the_same_bits(dev, kind):
    m, p, Y, want = _mixture(kind, np.random.RandomState(17), 10, 6, 90)
    plain = m.reconstruct(p, {"y": Y})
    _bits(m.reconstruct(p, {"y": Y}, exact=True), plain, kind)
    assert R.row_rel_err(plain, want) <= RTOL
