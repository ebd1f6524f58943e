"""Per-entry noise weights on the device: log_likelihood / reconstruct / sample_posterior / reconstruct_image
with ``my_data['weight']`` for BSC (with and without mu), MCA and MMCA -- against NumPy enumeration of the weighted joint,
against sums rebuilt from the returned candidates on truncated state sets (one case per instantiation and edge of the
kernels), the identities that tie the feature to code that exists (weights in {0, 1} are the masked call bit for bit, constant
weights the unweighted call at sigma / sqrt(c), integer weights the unweighted model with replicated dimensions), invariance
under whatever the zero-weight entries hold, bit for bit repeatable (calls, builds, row order, shards, chunks), an undisturbed
training run, the image path.  NumPy reference: tests/weighted_reference.py (pinned on the CPU by tests/test_weighted_cpu.py).

Tolerances: those of tests/test_masked_gpu.py.  Reconstructions and draws: |delta| / max_d |yhat_nd| <= 1e-11 per row.
Log-likelihoods: rtol = 1e-11; a row whose weights are all 0 at the full state set has the value log sum_s p(s) = 0 and is
compared on the scale of the terms that cancel in it, 1e-11 |c0|, c0 = H log(1 - pi).  Variances: the project's bound for V,
max_d |V - V_ref| <= 4e-11 max_d E_ref[ybar_d^2] per row (tests/test_reconstruct_var_gpu.py derives it from the 1e-11 on
yhat); the figure relative to max_d V is printed beside it.

Weights: 30 % zeros, the rest uniform in [0.25, 4]; row 0 all ones, row 1 all zeros, and one dimension zero in every other row
(row 0 keeps its ones: a row of ones and a dimension that is zero in EVERY row exclude each other)."""
import numpy as np
import pytest

import patches_reference as P
import patches_weighted_reference as PW
import recon_reference as R
import sample_reference as SR
import weighted_reference as WR
from test_masked_gpu import _entries, _problem, _ref_kind, _same_bits

pytestmark = pytest.mark.gpu

RTOL = 1e-11
VTOL = 4e-11
GAP = 1e-9
KINDS = ["bsc", "bsc_mu", "mca", "mmca"]


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def _weights(rng, N, D):
    Om = np.where(rng.uniform(size=(N, D)) < 0.3, 0.0, rng.uniform(0.25, 4.0, size=(N, D)))
    if D > 1:
        Om[:, D // 2] = 0.0
    Om[0] = 1.0
    if N > 1:
        Om[1] = 0.0
    return Om


def _check_rows(tag, got, want):
    err = R.row_rel_err(got, want)
    print("weighted %-44s row-relative error %.3e (bound %.1e)" % (tag, err, RTOL))
    assert got.shape == want.shape and got.dtype == np.float64
    assert err <= RTOL, (tag, err)


def _check_var(tag, got, want_v, want_y):
    m2 = (want_v + want_y ** 2).max(axis=1)
    err = np.abs(got - want_v).max(axis=1)
    vmax = want_v.max(axis=1)
    print("weighted %-44s variance: largest |delta| / max E[ybar^2] %.3e (bound %.1e); / max V %.3e" % (
        tag, float((err / np.where(m2 > 0, m2, 1.0)).max()), VTOL, float((err / np.where(vmax > 0, vmax, 1.0)).max())))
    assert got.shape == want_v.shape and (got >= 0).all()
    assert (err <= VTOL * m2).all(), tag


def _check_ll(tag, got, want, Om, p, H, full):
    got, want = np.asarray(got), np.asarray(want)
    empty = ~(np.asarray(Om) > 0).any(axis=1) if full else np.zeros(len(want), dtype=bool)
    c0 = abs(H * np.log(1. - float(p["pi"])))
    bound = np.where(empty, RTOL * c0, RTOL * np.abs(want))
    err = np.abs(got - want)
    print("weighted %-44s log_likelihood: largest |delta| / bound %.3e" % (tag, float((err / bound).max())))
    assert got.shape == want.shape
    assert (err <= bound).all(), (tag, float((err / bound).max()))


def _capture(m):
    """The model's weighted-evaluation hook, wrapped to keep what it returned."""
    kept = {}
    orig = m._obs_estep

    def hook(*a):
        kept["out"] = orig(*a)
        return kept["out"]
    m._obs_estep = hook
    return kept


def _gap(kind, p, Y, Om, Hp, tag):
    """The precondition of every exact candidate comparison, asserted on the reference: every row with a positive weight
    has the H'-th and (H'+1)-th score further apart than two f64 evaluations of them can differ."""
    sc, largest = WR.model_scores(_ref_kind(kind), p, Y, Om)
    rows = (Om > 0).any(axis=1)
    gap = WR.boundary_gap(sc, Hp, largest)[rows]
    print("weighted selection %-34s smallest boundary gap %.3e (needs > %.1e)" % (tag, gap.min(), GAP))
    assert gap.size == rows.sum() and (gap > GAP).all(), (tag, gap.min())


# ------------------------------------------------------------------------------------------------------- 1: enumeration
@pytest.mark.parametrize("kind", KINDS)
def test_against_enumeration(dev, kind):
    """H = 6, D = 20, N = 37, H' = gamma = H: log-likelihood rows, reconstruction, variance and the mean of draws with fixed
    uniforms (the states the NumPy CDF of the reference's log-joints draws, tests/sample_reference.py)."""
    D, H, N, M = 20, 6, 37, 64
    rng = np.random.RandomState(121 + KINDS.index(kind))
    m, p, Y = _problem(kind, rng, D, H, N, H, H)
    Om = _weights(rng, N, D)
    Yg = np.where(Om > 0, Y, np.nan)
    p_in = {k: np.array(v, copy=True) for k, v in p.items()}
    rk = _ref_kind(kind)
    want_y, want_l, want_v = WR.enumerate_all(rk, p, Yg, Om)
    kept = _capture(m)
    got_y, got_v = m.reconstruct(p, {"y": Yg, "weight": Om}, variance=True)
    got_l = m.log_likelihood(p, {"y": Yg, "weight": Om}, per_datapoint=True)
    for k in p_in:
        np.testing.assert_array_equal(p[k], p_in[k])
    assert (m.Hprime, m.gamma) == (H, H)
    assert np.isfinite(got_y).all() and np.isfinite(got_l).all() and np.isfinite(got_v).all()
    _check_rows(kind + " enumeration", got_y, want_y)
    _check_var(kind + " enumeration", got_v, want_v, want_y)
    _check_ll(kind + " enumeration", got_l, want_l, Om, p, H, True)
    _same_bits(m.reconstruct(p, {"y": Yg, "weight": Om}), got_y, "Yhat of the call without variance=")
    tot = m.log_likelihood(p, {"y": Yg, "weight": Om})
    np.testing.assert_allclose(tot, got_l.sum(), rtol=1e-12)
    # a row of zero weights: the posterior is the prior over K_n, the candidates the H' largest indices
    cand = kept["out"]["cand"].cpu().numpy()
    assert sorted(cand[1]) == list(range(H))
    if kind.startswith("bsc"):
        np.testing.assert_array_equal(cand[1], np.arange(H))
    # draws: the reference's log-joints in the device's column order, uniforms moved off the reference's CDF edges
    lp, means = WR.joints_from_candidates(rk, p, Yg, Om, cand, m.state_matrix)
    U, _ = SR.nudge(rng.uniform(size=(N, M)), SR.cdfs(lp))
    idx = SR.draw_states(lp, U)
    assert (idx >= 0).all()
    want_s = np.array([means[n][idx[n]] for n in range(N)]).transpose(1, 0, 2)          # (M, N, D)
    got_s, lat = m.sample_posterior(p, {"y": Yg, "weight": Om}, n_samples=M, uniforms=U, latents=True)
    assert got_s.shape == (M, N, D) and lat.shape == (M, N, H) and np.isfinite(got_s).all()
    _check_rows(kind + " mean of %d draws" % M, got_s.mean(axis=0), want_s.mean(axis=0))
    _check_rows(kind + " every draw", got_s.reshape(M * N, D), want_s.reshape(M * N, D))
    states = [WR.truncated_states(H, c, m.state_matrix) for c in cand]
    want_lat = np.zeros((M, N, H))
    for n in range(N):
        for k in range(M):
            want_lat[k, n, list(states[n][idx[n, k]])] = 1.0
    np.testing.assert_array_equal(lat, want_lat)


# --------------------------------------------------------------------------------------------------------- 2: truncated
# One case per instantiation and edge, the shapes of DESIGN 4.16's table (dispatch is a function of H, D and H' alone):
#   bsc_obs_estep_kernel<VPL, double>   H = 65 / 130 / 257 / 520 / 1024: VPL 2, 4, 8, 16, 16; H' = 12 and 16: 66 and 120 pairs,
#                                       the second pair of a lane; D = 70: two slabs; D = 64 / 65: a full slab and a ragged
#                                       slab of one dimension; H = 1024 with H' = 16: both limits at once
#   mca_obs_estep_kernel<DPL, double>   D = 129 / 257 / 513: DPL 4, 8, 16; D = 1024 with H' = 16: the largest LDS request;
#                                       D = 64 / 128 / 256 / 512: full last slabs; D = 1: one-dimension rows
#   mca_weighted_select_scores_kernel   H = 65 and 130 (two and three H tiles), D across the 16-wide slabs
TRUNC = ([(k, D, H, Hp, g, 64) for k in ("bsc", "bsc_mu")
          for D, H, Hp, g in ((33, 65, 6, 3), (70, 130, 12, 3), (33, 257, 6, 3), (24, 520, 5, 2), (40, 1024, 16, 2),
                              (64, 24, 6, 3), (65, 24, 6, 3))] +
         [(k, D, H, Hp, g, 64) for k in ("mca", "mmca")
          for D, H, Hp, g in ((129, 24, 6, 3), (257, 65, 5, 2), (513, 130, 6, 3), (1024, 20, 16, 2), (64, 24, 6, 3),
                              (128, 24, 6, 3), (256, 24, 5, 2), (512, 20, 5, 2))] +
         [(k, 1, 8, 4, 2, 24) for k in ("mca", "mmca")])


def _weighted_entries(kind):
    if kind.startswith("bsc"):
        return {"pm_weighted_prepare_f64", "pm_bsc_weighted_estep_f64", "pm_recon_expect_f64"}
    sel = {"pm_mca_weighted_select_scores_f64"} if kind == "mca" else set()
    return sel | {"pm_weighted_prepare_f64", "pm_mca_weighted_estep_f64", "pm_recon_expect_f64", "pm_recon_mca_f64"}


@pytest.mark.parametrize("kind,D,H,Hp,g,N", TRUNC)
def test_truncated_candidates_and_sums(dev, kind, D, H, Hp, g, N):
    rng = np.random.RandomState(D + H + KINDS.index(kind))
    m, p, Y = _problem(kind, rng, D, H, N, Hp, g)
    Om = _weights(rng, N, D)
    Yg = np.where(Om > 0, Y, 1e300)
    rk = _ref_kind(kind)
    tag = "%s D=%d H=%d H'=%d" % (kind, D, H, Hp)
    if D > 1:
        _gap(kind, p, Yg, Om, Hp, tag)
    # (D = 1: a score is ONE term with nothing to sum -- both sides hold the same bits, zeros tie exactly and the index rule
    # decides them on both sides)
    kept = _capture(m)
    calls = _entries(m)
    got_y = m.reconstruct(p, {"y": Yg, "weight": Om})
    assert _weighted_entries(kind) <= set(calls) and not [c for c in calls if "masked" in c], calls
    cand = kept["out"]["cand"].cpu().numpy()
    assert cand.shape == (N, Hp)
    np.testing.assert_array_equal(cand, WR.select(rk, p, Yg, Om, Hp))
    if kind.startswith("bsc"):
        np.testing.assert_array_equal(cand[1], np.arange(H - Hp, H))      # zero weights: the H' largest indices
    want_y, want_l, _ = WR.from_candidates(rk, p, Yg, Om, cand, m.state_matrix)
    _check_rows(tag, got_y, want_y)
    del calls[:]
    got_l = m.log_likelihood(p, {"y": Yg, "weight": Om}, per_datapoint=True)
    assert (_weighted_entries(kind) - {"pm_recon_expect_f64", "pm_recon_mca_f64"}) <= set(calls), calls
    np.testing.assert_array_equal(kept["out"]["cand"].cpu().numpy(), cand)
    _check_ll(tag, got_l, want_l, Om, p, H, False)      # (a truncated set's prior mass is below 1: no computed zero)


# ------------------------------------------------------------------------------- 2b: second trip of the grid-stride loops
@pytest.mark.parametrize("kind", ["bsc", "mca"])
def test_second_trip_of_the_row_loops(dev, kind):
    """N = 8269: at most 2048 workgroups of four rows, so row 8192 starts the second trip of every row loop (prepare, the row
    kernels).  The rows from 150 before the boundary onwards against the NumPy sums over the device's candidates; the whole
    result bit for bit against the same calls on shards of 4096 rows.  (D = 16: at D = 8 with 30 % zero weights some rows keep
    one or two dimensions and several MCA scores are exactly 0 -- an exact tie at the selection boundary.)"""
    D, H, Hp, g, N = 16, 6, 3, 2, 8269
    rng = np.random.RandomState(N % 1000 + KINDS.index(kind))
    m, p, Y = _problem(kind, rng, D, H, N, Hp, g)
    Om = _weights(rng, N, D)
    Yg = np.where(Om > 0, Y, np.nan)
    kept = _capture(m)
    got_y = m.reconstruct(p, {"y": Yg, "weight": Om})
    cand = kept["out"]["cand"].cpu().numpy()
    got_l = m.log_likelihood(p, {"y": Yg, "weight": Om}, per_datapoint=True)
    assert got_y.shape == (N, D) and np.isfinite(got_y).all() and np.isfinite(got_l).all()
    rows = np.arange(8192 - 150, N)
    _gap(kind, p, Yg[rows], Om[rows], Hp, "%s N=%d tail" % (kind, N))
    np.testing.assert_array_equal(cand[rows], WR.select(kind, p, Yg[rows], Om[rows], Hp))
    want_y, want_l, _ = WR.from_candidates(kind, p, Yg[rows], Om[rows], cand[rows], m.state_matrix)
    _check_rows("%s N=%d second trip" % (kind, N), got_y[rows], want_y)
    _check_ll("%s N=%d second trip" % (kind, N), got_l[rows], want_l, Om[rows], p, H, False)
    parts = [(m.reconstruct(p, {"y": Yg[i:i + 4096], "weight": Om[i:i + 4096]}),
              m.log_likelihood(p, {"y": Yg[i:i + 4096], "weight": Om[i:i + 4096]}, per_datapoint=True))
             for i in range(0, N, 4096)]
    _same_bits(np.concatenate([a for a, _ in parts]), got_y, "reconstruct in shards")
    _same_bits(np.concatenate([b for _, b in parts]), got_l, "log_likelihood in shards")


# ------------------------------------------------------------------------------------------------------------ 2c: limits
@pytest.mark.parametrize("kind,D,H,Hp", [("bsc", 16, 1025, 4), ("bsc", 16, 40, 17), ("mca", 1025, 12, 4), ("mca", 16, 40, 17),
                                          ("mmca", 1025, 12, 4)])
def test_one_past_a_limit_raises(dev, kind, D, H, Hp):
    """HipError -- the library's PM_ERANGE or the host's own range check (some in the constructor) -- and no result."""
    from prosper_amd import _lib
    rng = np.random.RandomState(D + H + Hp)
    N = 12
    with pytest.raises(_lib.HipError):
        m, p, Y = _problem(kind, rng, D, H, N, Hp, 2)
        m.reconstruct(p, {"y": Y, "weight": _weights(rng, N, D)})
    with pytest.raises(_lib.HipError):
        m, p, Y = _problem(kind, rng, D, H, N, Hp, 2)
        m.log_likelihood(p, {"y": Y, "weight": _weights(rng, N, D)}, per_datapoint=True)


# -------------------------------------------------------------------------------------------------------- 3: identities
@pytest.mark.parametrize("kind", KINDS)
def test_zero_one_weights_return_the_bits_of_the_masked_call(dev, kind):
    D, H, Hp, g, N, M = 70, 24, 6, 3, 130, 3
    rng = np.random.RandomState(140 + KINDS.index(kind))
    m, p, Y = _problem(kind, rng, D, H, N, Hp, g)
    mask = rng.uniform(size=(N, D)) < 0.5
    mask[0], mask[1], mask[:, 7] = True, False, False
    Yg = np.where(mask, Y, np.nan)
    Om = mask.astype(np.float64)
    U = rng.uniform(size=(N, M))
    a, b = {"y": Yg, "weight": Om}, {"y": Yg, "mask": mask}
    _same_bits(m.log_likelihood(p, a, per_datapoint=True), m.log_likelihood(p, b, per_datapoint=True), "log-likelihood rows")
    assert m.log_likelihood(p, a) == m.log_likelihood(p, b)
    _same_bits(m.reconstruct(p, a), m.reconstruct(p, b), "reconstruct")
    (ya, va), (yb, vb) = m.reconstruct(p, a, variance=True), m.reconstruct(p, b, variance=True)
    _same_bits(ya, yb, "reconstruct with variance")
    _same_bits(va, vb, "variance")
    (sa, la), (sb, lb) = (m.sample_posterior(p, d, n_samples=M, uniforms=U, latents=True) for d in (a, b))
    _same_bits(sa, sb, "draws")
    _same_bits(la, lb, "latents of the draws")


CONST = {"bsc": (70, 24, 6, 3), "bsc_mu": (70, 8, 8, 8), "mca": (70, 24, 6, 3), "mmca": (70, 24, 6, 3)}


@pytest.mark.parametrize("c", [0.37, 5.0])
@pytest.mark.parametrize("kind", KINDS)
def test_constant_weights_equal_the_unweighted_call_at_sigma_over_sqrt_c(dev, kind, c):
    """The existing, trusted unweighted path at sigma / sqrt(c) is the reference; the log-likelihood matches with its
    constant: -D/2 log(2 pi sigma^2) + D/2 log c.  (BSC with mu at H' = gamma = H: the unweighted selection ranks the uncentred
    <W_h, y> / |W_h|, the weighted one b_h = <W_h, y - mu> -- tests/test_masked_gpu.py, shared mask.)"""
    (D, H, Hp, g), N = CONST[kind], 130
    rng = np.random.RandomState(160 + KINDS.index(kind))
    m, p, Y = _problem(kind, rng, D, H, N, Hp, g)
    Om = np.full((N, D), c)
    if Hp < H:
        _gap(kind, p, Y, Om, Hp, "%s c=%g" % (kind, c))
    q = dict(p, sigma=p["sigma"] / np.sqrt(c))
    tag = "%s omega = %g" % (kind, c)
    _check_rows(tag, m.reconstruct(p, {"y": Y, "weight": Om}), m.reconstruct(q, {"y": Y}))
    got_l = m.log_likelihood(p, {"y": Y, "weight": Om}, per_datapoint=True)
    want_l = m.log_likelihood(q, {"y": Y}, per_datapoint=True)
    _check_ll(tag, got_l, want_l, Om, p, H, False)
    np.testing.assert_allclose(m.log_likelihood(p, {"y": Y, "weight": Om}), m.log_likelihood(q, {"y": Y}), rtol=RTOL)


@pytest.mark.parametrize("kind", KINDS)
def test_integer_weights_equal_the_model_with_replicated_dimensions(dev, kind):
    """One weight vector in {0, 1, 2, 3} for all rows: the unweighted model whose row d of W (and of mu) and entry d of y
    appear omega_d times has the same posterior, so its reconstruction agrees at the original dimensions with a positive
    weight.  Its selection scores are the weighted ones (sum_d omega_d ... = the sum over the copies), so the candidates agree
    where the boundary gap is above rounding -- asserted on the reference."""
    (D, H, Hp, g), N = CONST[kind], 130
    rng = np.random.RandomState(180 + KINDS.index(kind))
    m, p, Y = _problem(kind, rng, D, H, N, Hp, g)
    om = rng.randint(0, 4, size=D)
    om[:4] = [0, 1, 2, 3]
    Om = np.tile(om.astype(np.float64), (N, 1))
    if Hp < H:
        _gap(kind, p, Y, Om, Hp, kind + " integer weights")
    rep = np.repeat(np.arange(D), om)                           # dimension d, omega_d times
    first = np.array([int(np.nonzero(rep == d)[0][0]) for d in np.nonzero(om)[0]])
    big = type(m)(len(rep), H, Hp, g)
    q = dict(p, W=p["W"][rep])
    if "mu" in p:
        q["mu"] = p["mu"][rep]
    want = big.reconstruct(q, {"y": Y[:, rep]})[:, first]
    got = m.reconstruct(p, {"y": np.where(Om > 0, Y, np.inf), "weight": Om.astype(np.int64)})[:, om > 0]
    _check_rows(kind + " integer weights", got, want)


# ---------------------------------------------------------------------------------------------------------------- 4: bits
@pytest.mark.parametrize("kind", KINDS)
def test_zero_weight_entries_change_no_bit(dev, kind):
    D, H, Hp, g, N, M = 23, 12, 5, 3, 90, 2
    rng = np.random.RandomState(60 + KINDS.index(kind))
    m, p, Y = _problem(kind, rng, D, H, N, Hp, g)
    Om = _weights(rng, N, D)
    U = rng.uniform(size=(N, M))
    on = Om > 0

    def run(Yf):
        d = {"y": Yf, "weight": Om}
        y, v = m.reconstruct(p, d, variance=True)
        return (y, v, m.log_likelihood(p, d, per_datapoint=True), np.array([m.log_likelihood(p, d)]),
                m.sample_posterior(p, d, n_samples=M, uniforms=U))
    base = run(np.where(on, Y, 0.0))
    assert all(np.isfinite(x).all() for x in base)
    for fill in (np.nan, np.inf, 1e300):
        for x, y0, what in zip(run(np.where(on, Y, fill)), base, ("reconstruct", "variance", "rows", "total", "draws")):
            _same_bits(x, y0, "%s, fill %r" % (what, fill))
    # a NaN at an entry with a positive weight: that row is NaN and no other row moves
    n = 7
    d = int(np.nonzero(on[n])[0][0])
    Yn = np.where(on, Y, np.nan)
    Yn[n, d] = np.nan
    got = run(Yn)
    assert np.isnan(got[0][n]).all() and np.isnan(got[2][n])
    for x, y0 in zip(got[:3], base[:3]):
        _same_bits(np.delete(x, n, axis=0), np.delete(y0, n, axis=0), "other rows")


@pytest.mark.parametrize("kind", KINDS)
def test_bits_repeat_across_calls_builds_row_order_shards_and_weight_types(dev, kind):
    import torch
    from prosper_amd.em.camodels._device import DeviceArray
    D, H, Hp, g, N = 24, 12, 5, 3, 700
    rng = np.random.RandomState(80 + KINDS.index(kind))
    m, p, Y = _problem(kind, rng, D, H, N, Hp, g)
    Om = _weights(rng, N, D)
    Om = np.where(rng.uniform(size=Om.shape) < 0.5, Om, np.float32(Om).astype(np.float64))   # (half of them exact in f32)
    a = m.reconstruct(p, {"y": Y, "weight": Om})
    l = m.log_likelihood(p, {"y": Y, "weight": Om}, per_datapoint=True)
    t = m.log_likelihood(p, {"y": Y, "weight": Om})
    _same_bits(m.reconstruct(p, {"y": Y, "weight": Om}), a, "second call")
    _same_bits(m.log_likelihood(p, {"y": Y, "weight": Om}, per_datapoint=True), l, "second call")
    d = m.reconstruct(p, {"y": Y, "weight": Om}, device=True)
    assert isinstance(d, DeviceArray) and d.tensor.is_cuda
    _same_bits(np.asarray(d), a, "device output")
    m.deterministic = True
    _same_bits(m.reconstruct(p, {"y": Y, "weight": Om}), a, "deterministic build")
    _same_bits(m.log_likelihood(p, {"y": Y, "weight": Om}, per_datapoint=True), l, "deterministic build")
    assert m.log_likelihood(p, {"y": Y, "weight": Om}) == t
    m.deterministic = False
    perm = rng.permutation(N)
    _same_bits(m.reconstruct(p, {"y": Y[perm], "weight": Om[perm]}), a[perm], "row permutation")
    _same_bits(m.log_likelihood(p, {"y": Y[perm], "weight": Om[perm]}, per_datapoint=True), l[perm], "row permutation")
    _same_bits(m.reconstruct(p, {"y": Y[130:333], "weight": Om[130:333]}), a[130:333], "shard")
    _same_bits(m.log_likelihood(p, {"y": Y[130:333], "weight": Om[130:333]}, per_datapoint=True), l[130:333], "shard")
    _same_bits(m.reconstruct(p, {"y": Y[5:6], "weight": Om[5:6]}), a[5:6], "one row")
    # the weight's types: NumPy, torch (host and device; a float64 device tensor with its own leading dimension is used in
    # place), DeviceArray; float32 and integers are converted once
    wide = torch.zeros((N, D + 9), dtype=torch.float64, device=dev)
    wide[:, :D] = torch.from_numpy(Om).to(dev)
    for what, wg in (("torch host", torch.from_numpy(Om)), ("torch device", torch.from_numpy(Om).to(dev)),
                     ("device view with its own leading dimension", wide[:, :D]),
                     ("DeviceArray", DeviceArray(torch.from_numpy(Om).to(dev))),
                     ("transposed storage", torch.from_numpy(np.ascontiguousarray(Om.T)).to(dev).t())):
        _same_bits(m.reconstruct(p, {"y": Y, "weight": wg}), a, what)
    O32 = np.float32(Om)
    a32 = m.reconstruct(p, {"y": Y, "weight": O32.astype(np.float64)})
    _same_bits(m.reconstruct(p, {"y": Y, "weight": O32}), a32, "float32")
    _same_bits(m.reconstruct(p, {"y": Y, "weight": torch.from_numpy(O32).to(dev)}), a32, "float32 on the device")
    Oi = np.round(Om).astype(np.int32)
    _same_bits(m.reconstruct(p, {"y": Y, "weight": Oi}), m.reconstruct(p, {"y": Y, "weight": Oi.astype(np.float64)}), "int32")
    # refused on the device as on the host: one reduction, before any launch
    calls = _entries(m)
    bad = torch.from_numpy(Om).to(dev).clone()
    bad[3, 2] = float("nan")
    for entry in (m.reconstruct, m.log_likelihood, m.sample_posterior):
        with pytest.raises(ValueError, match="weight"):
            entry(p, {"y": Y, "weight": bad})
    bad[3, 2] = -0.5
    with pytest.raises(ValueError, match="weight"):
        m.reconstruct(p, {"y": Y, "weight": DeviceArray(bad)})
    assert not calls, calls
    # calls without the key run the entries of the unweighted call, and none of the new ones
    m.reconstruct(p, {"y": Y})
    m.log_likelihood(p, {"y": Y})
    plain = list(calls)
    assert plain and not [c for c in plain if "weighted" in c or "masked" in c], plain
    fresh = _problem(kind, np.random.RandomState(0), D, H, 4, Hp, g)[0]
    calls2 = _entries(fresh)
    fresh.reconstruct(p, {"y": Y})
    fresh.log_likelihood(p, {"y": Y})
    # (a model that never saw a weight launches the same entries; the norms of a shard that is already resident are kept)
    assert set(calls2) - {"pm_row_sqnorm_f64"} == set(plain) - {"pm_row_sqnorm_f64"}, (calls2, plain)
    del calls[:]
    m.reconstruct(p, {"y": Y, "weight": Om})
    assert [c for c in calls if "weighted" in c] and "pm_gemm_nt_rows_f64" in calls, calls
    assert not [c for c in calls if c in ("pm_gemm_nt_f64", "pm_gemm_nt_small_f64") or "masked" in c], calls


# ------------------------------------------------------------------------------------------- 5: training undisturbed
def _schedule(steps):
    from prosper_amd.em.annealing import LinearAnnealing
    a = LinearAnnealing(steps)
    a["T"] = [(0, 2.), (.7, 1.)]
    a["Ncut_factor"] = [(0, 0.), (2. / 3, 1.)]
    a["anneal_prior"] = False
    a.as_dict = lambda: {k: a[k] for k in ("T", "Ncut_factor")}
    return a


def _train(m, params, Y, Yh, Oh, steps, interleave):
    a = _schedule(steps)
    for _ in range(steps):
        params = m.step(a, params, {"y": Y})
        if interleave:
            hp = (m.Hprime, m.gamma)
            q = {k: np.array(v, copy=True) for k, v in params.items()}
            out = m.reconstruct(q, {"y": Yh, "weight": Oh})
            ll = m.log_likelihood(q, {"y": Yh, "weight": Oh})
            dr = m.sample_posterior(q, {"y": Yh, "weight": Oh}, seed=1)
            assert out.shape == Yh.shape and np.isfinite(out).all() and np.isfinite(ll) and np.isfinite(dr).all()
            assert (m.Hprime, m.gamma) == hp
            for k in q:
                np.testing.assert_array_equal(q[k], params[k])
        a.next()
    return {k: np.array(v, copy=True) for k, v in params.items()}, getattr(m, "spec_hits", None)


@pytest.mark.parametrize("kind", ["bsc", "mca"])
def test_training_undisturbed(dev, kind):
    rng = np.random.RandomState(14)
    D, H, N, Nh = 20, 10, 900, 200
    _, p, Y = _problem(kind, rng, D, H, N + Nh, 5, 3)
    p = dict(p, W=p["W"] * rng.uniform(0.9, 1.1, size=p["W"].shape))
    Yt, Yh = Y[:N], Y[N:]
    Oh = _weights(rng, Nh, D)

    def det():
        m = _problem(kind, np.random.RandomState(0), D, H, 4, 5, 3)[0]
        m.deterministic = True
        return m
    ref, hits_ref = _train(det(), {k: np.array(v, copy=True) for k, v in p.items()}, Yt, Yh, Oh, 5, False)
    got, hits_got = _train(det(), {k: np.array(v, copy=True) for k, v in p.items()}, Yt, Yh, Oh, 5, True)
    for k in ref:
        np.testing.assert_array_equal(ref[k], got[k], err_msg=k)
    if kind == "bsc":
        assert hits_ref is not None and hits_ref == hits_got, (hits_ref, hits_got)


# ---------------------------------------------------------------------------------------------------------------- 6: image
PB = 4


def _image_problem(kind, seed):
    """A 23 x 19 image (a stack of two for MCA) of patches drawn from the model at H' = 5, gamma = 3, with a weight image."""
    rng = np.random.RandomState(seed)
    m, p, _ = _problem(kind, rng, PB * PB, 8, 4, 5, 3)
    shape = (23, 19) if kind != "mca" else (2, 23, 19)
    img = rng.normal(size=shape) * 1.5 + (1.0 if kind == "mca" else 0.0)
    w = np.where(rng.uniform(size=shape) < 0.3, 0.0, rng.uniform(0.25, 4.0, size=shape))
    return m, p, img, w


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("kind", ["bsc_mu", "mca"])
def test_image_is_the_loop_over_patches_and_bits_do_not_depend_on_chunk(dev, kind, stride):
    from prosper_amd.utils import patches as U
    m, p, img, w = _image_problem(kind, 200 + stride)
    holes = np.where(w > 0, img, np.nan)
    got = m.reconstruct_image(p, holes, weight=w, stride=stride)
    assert got.shape == img.shape and got.dtype == np.float64 and np.isfinite(got).all()
    # the plain NumPy loop over patches through reconstruct(), averaged
    Yp, Wp = P.extract(holes, (PB, PB), stride), P.extract(w, (PB, PB), stride)
    est, V = m.reconstruct(p, {"y": Yp, "weight": Wp}, variance=True)
    want = P.average(est, img.shape, (PB, PB), stride)
    err = np.abs(got - want).max() / np.abs(want).max()
    print("weighted reconstruct_image %s stride %d against the loop over patches: %.3e of max |image| (bound %.1e)" % (
        kind, stride, err, RTOL))
    assert err <= RTOL, err
    # aggregate='precision': tests/patches_weighted_reference.py fed with the weighted per-patch estimates
    floor = U.PRECISION_FLOOR * float(p["sigma"]) ** 2
    gp, gv = m.reconstruct_image(p, holes, weight=w, stride=stride, aggregate="precision", variance=True)
    wp = PW.average(est, img.shape, (PB, PB), stride, wgt=V, wmode=1, floor=floor)
    wv = PW.weighted_variance(V, img.shape, (PB, PB), stride, floor)
    err = np.abs(gp - wp).max() / np.abs(wp).max()
    errv = np.abs(gv - wv).max() / np.abs(wv).max()
    print("weighted reconstruct_image %s stride %d precision aggregate: %.3e of max |image|, variance map %.3e (bound %.1e, "
          "%.1e)" % (kind, stride, err, errv, RTOL, VTOL))
    assert err <= RTOL and errv <= VTOL, (err, errv)
    # bits: chunks, both aggregates, the builds, whatever the image holds at weight 0, window and variance
    nc = len(P.starts(19, PB, stride))
    win = np.outer(np.hanning(PB + 2)[1:-1], np.hanning(PB + 2)[1:-1])
    base = {"mean": got, "precision": gp}
    for agg in ("mean", "precision"):
        for chunk in (nc, 7 * nc + 3):
            _same_bits(U.denoise_image(m, p, holes, stride=stride, chunk=chunk, weight=w, aggregate=agg), base[agg],
                       "%s chunk %d" % (agg, chunk))
        _same_bits(m.reconstruct_image(p, np.where(w > 0, img, 1e300), weight=w, stride=stride, aggregate=agg), base[agg],
                   agg + " fill")
        ww = m.reconstruct_image(p, holes, weight=w, stride=stride, aggregate=agg, window=win, variance=True)
        wc = U.denoise_image(m, p, holes, stride=stride, aggregate=agg, window=win, variance=True, weight=w, chunk=3 * nc)
        _same_bits(ww[0], wc[0], agg + " window, chunk")
        _same_bits(ww[1], wc[1], agg + " window variance map, chunk")
    m.deterministic = True
    try:
        _same_bits(m.reconstruct_image(p, holes, weight=w, stride=stride, chunk=5 * nc), got, "deterministic build")
    finally:
        m.deterministic = False
    # weights in {0, 1}: the masked image call, bit for bit
    mask = w > 0
    _same_bits(m.reconstruct_image(p, holes, weight=mask.astype(np.float32), stride=stride),
               m.reconstruct_image(p, holes, mask=mask, stride=stride), "0 / 1 weights against the mask")


def test_weighting_helps_where_the_noise_varies(dev):
    """Bars at their generating parameters, noise standard deviation rising 4 x from left to right, weights = mean noise
    variance / pixel noise variance and sigma = the root of the mean variance: the weighted estimate has the smaller error --
    first on the NumPy reference (a failure there blames the inputs), then on the device."""
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    rng = np.random.RandomState(5)
    a, pi, H = 3.0, 0.2, 2 * PB
    clean, _, _, _ = P.bars_image(rng, 24, 24, a, pi, 1.0)
    sd = np.tile(np.linspace(0.5, 2.0, 24)[None, :], (24, 1))
    noisy = clean + sd * rng.normal(size=clean.shape)
    mv = float((sd ** 2).mean())
    w = mv / sd ** 2
    p = {"W": P.bars_W(PB, a), "pi": pi, "sigma": np.sqrt(mv)}
    m = BSC_ET(PB * PB, H, H, H)
    Yp, Wp = P.extract(noisy, (PB, PB), 2), P.extract(w, (PB, PB), 2)
    ref_w = P.average(WR.enumerate_all("bsc", p, Yp, Wp)[0], clean.shape, (PB, PB), 2)
    ref_u = P.average(WR.enumerate_all("bsc", p, Yp, np.ones_like(Wp))[0], clean.shape, (PB, PB), 2)
    got_w = m.reconstruct_image(p, noisy, weight=w, stride=2)
    got_u = m.reconstruct_image(p, noisy, stride=2)
    mse = lambda x: float(((x - clean) ** 2).mean())
    print("noise ramp 4 x: MSE noisy %.4f, unweighted %.4f (numpy %.4f), weighted %.4f (numpy %.4f)" % (
        mse(noisy), mse(got_u), mse(ref_u), mse(got_w), mse(ref_w)))
    assert mse(ref_w) < mse(ref_u) < mse(noisy)
    assert mse(got_w) < mse(got_u) < mse(noisy)
    assert np.abs(got_w - ref_w).max() <= RTOL * np.abs(ref_w).max()


# ------------------------------------------------------------------------------------------------------------ 7: refusals
def test_refusals(dev):
    from prosper_amd import _lib
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    from prosper_amd.em.camodels.dsc_et import DSC_ET
    from prosper_amd.em.camodels.tsc_et import TSC_ET
    from prosper_amd.em.camodels.gsc_et import GSC
    from prosper_amd.em.mixturemodels.MoG import MoG
    from prosper_amd.em.mixturemodels.MoP import MoP
    rng = np.random.RandomState(3)
    D, H, N = 16, 8, 20
    Y, Om = rng.normal(size=(N, D)), _weights(rng, N, D)
    p = {"W": rng.normal(size=(D, H)), "pi": 0.2, "sigma": 1.0}
    for m in (DSC_ET(D, H, 4, 2), TSC_ET(D, H, 4, 2), GSC(D, H, 4, 2), MoG(D, H), MoP(D, H)):
        calls = _entries(m) if hasattr(m, "_call") else []
        for call in (lambda: m.reconstruct(p, {"y": Y, "weight": Om}), lambda: m.log_likelihood(p, {"y": Y, "weight": Om}),
                     lambda: m.sample_posterior(p, {"y": Y, "weight": Om}),
                     lambda: m.reconstruct_image(p, rng.normal(size=(9, 9)), weight=np.ones((9, 9)), patch=4)):
            with pytest.raises(NotImplementedError, match="(?s)%s.*weight" % type(m).__name__):
                call()
        assert not calls, (type(m).__name__, calls)
    m = BSC_ET(D, H, 4, 2)
    calls = _entries(m)
    with pytest.raises(NotImplementedError, match="exact"):
        m.log_likelihood(p, {"y": Y, "weight": Om}, exact=True)
    with pytest.raises(ValueError, match="center"):
        m.reconstruct_image(p, rng.normal(size=(9, 9)), weight=np.ones((9, 9)), center=True)
    with pytest.raises(ValueError, match="weight"):
        m.reconstruct_image(p, rng.normal(size=(9, 9)), weight=np.ones((9, 8)))
    with pytest.raises(ValueError, match="(?s)weight.*mask"):
        m.reconstruct(p, {"y": Y, "weight": Om, "mask": Om > 0})
    for bad in (Om[:, :-1], Om[:-1], Om.ravel(), Om[:, :, None], -Om, np.where(Om > 1, np.inf, Om)):
        with pytest.raises(ValueError, match="weight"):
            m.reconstruct(p, {"y": Y, "weight": bad})
        with pytest.raises(ValueError, match="weight"):
            m.log_likelihood(p, {"y": Y, "weight": bad})
    for f in (lambda: m.step(_schedule(3), p, {"y": Y, "weight": Om}), lambda: m.E_step(_schedule(3), p, {"y": Y, "weight": Om}),
              lambda: m.select_Hprimes(p, {"y": Y, "weight": Om})):
        with pytest.raises(NotImplementedError, match="weight"):
            f()
    big = BSC_ET(D, 20, 17, 2)
    with pytest.raises(_lib.HipError, match="16"):
        big.reconstruct({"W": rng.normal(size=(D, 20)), "pi": 0.1, "sigma": 1.0}, {"y": Y, "weight": Om})
    assert not calls, calls
    # the model still works afterwards
    assert np.isfinite(m.reconstruct(p, {"y": Y, "weight": Om})).all()
