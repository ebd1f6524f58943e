"""Missing values on the device: log_likelihood / reconstruct / reconstruct_image with ``my_data['mask']`` for
BSC (with and without mu), MCA and MMCA -- against NumPy enumeration of the masked joint, against sums rebuilt from the
returned candidates on truncated state sets, against the unmasked calls of the sub-model, invariance under whatever the
unobserved entries hold, bit for bit repeatable (calls, builds, row order, shards), an undisturbed training run, the image
path and the refusals.  NumPy reference: tests/masked_reference.py (pinned on the CPU by tests/test_masked_cpu.py).

Tolerances.  Reconstructions: the project's bound for per-row values against NumPy, |delta| / max_d |yhat_nd| <= 1e-11 per
row (tests/test_reconstruct_gpu.py).  Log-likelihoods: rtol = 1e-11, what tests/test_loglik_gpu.py holds against NumPy.  One
row needs a word: with nothing observed and the full state set the value is log sum_s p(s) = 0 -- the NumPy reference
itself returns a rounding residue of ~1e-16 there, and no relative bound on a computed zero can hold; such a row is compared
on the scale of the terms that cancel in it, 1e-11 |c0| with c0 = H log(1 - pi) (the row's value is lse + c0)."""
import numpy as np
import pytest

import masked_reference as MR
import patches_reference as P
import recon_reference as R

pytestmark = pytest.mark.gpu

RTOL = 1e-11
KINDS = ["bsc", "bsc_mu", "mca", "mmca"]


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def _ref_kind(kind):
    return "bsc" if kind.startswith("bsc") else kind


def _problem(kind, rng, D, H, N, Hp, g):
    """(model, params, Y): continuous random data drawn from the parameters the call is given (no ties)."""
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    from prosper_amd.em.camodels.mca_et import MCA_ET
    from prosper_amd.em.camodels.mmca_et import MMCA_ET
    S = rng.uniform(size=(N, H)) < min(0.3, 2.5 / H)
    if kind.startswith("bsc"):
        p = {"W": rng.normal(size=(D, H)), "pi": min(0.3, 2.5 / H), "sigma": 1.3}
        if kind == "bsc_mu":
            p["mu"] = rng.normal(size=D)
        Y = S @ p["W"].T + p.get("mu", 0.0) + p["sigma"] * rng.normal(size=(N, D))
        return BSC_ET(D, H, Hp, g), p, Y
    signed = kind == "mmca"
    W = rng.uniform(-2, 3, size=(D, H)) if signed else rng.uniform(0.1, 3, size=(D, H))
    W = np.where(np.abs(W) < 0.05, 0.05, W)
    p = {"W": W, "pi": min(0.25, 2.5 / H), "sigma": 0.7}
    mean = R.mca_mean(W, 6.0 if signed else 21.0, signed)
    Y = np.array([mean(np.nonzero(s)[0]) for s in S]) + p["sigma"] * rng.normal(size=(N, D))
    return (MMCA_ET if signed else MCA_ET)(D, H, Hp, g), p, Y


def _mask(rng, N, D, frac=0.5):
    """Random mask with ``frac`` observed; row 0 fully observed, row 1 not at all."""
    M = rng.uniform(size=(N, D)) < frac
    M[0] = True
    if N > 1:
        M[1] = False
    return M


def _check_rows(tag, got, want):
    err = R.row_rel_err(got, want)
    print("masked reconstruct %-34s row-relative error %.3e (bound %.1e)" % (tag, err, RTOL))
    assert got.shape == want.shape and got.dtype == np.float64
    assert err <= RTOL, (tag, err)


def _check_ll(tag, got, want, M, p, H):
    got, want = np.asarray(got), np.asarray(want)
    empty = ~np.asarray(M).any(axis=1)
    c0 = abs(H * np.log(1. - float(p["pi"])))
    bound = np.where(empty, RTOL * c0, RTOL * np.abs(want))
    err = np.abs(got - want)
    print("masked log_likelihood %-31s largest |delta| / bound %.3e" % (tag, float((err / bound).max())))
    assert got.shape == want.shape
    assert (err <= bound).all(), (tag, float((err / bound).max()))


def _capture(m):
    """The model's masked-evaluation hook, wrapped to keep what it returned."""
    kept = {}
    orig = m._obs_estep

    def hook(*a):
        kept["out"] = orig(*a)
        return kept["out"]
    m._obs_estep = hook
    return kept


def _same_bits(a, b, what=""):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, what
    assert np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64)), what


# ------------------------------------------------------------------------------------------------------- 1: enumeration
@pytest.mark.parametrize("kind", KINDS)
def test_against_enumeration(dev, kind):
    D, H, N = 20, 6, 37
    rng = np.random.RandomState(21 + KINDS.index(kind))
    m, p, Y = _problem(kind, rng, D, H, N, H, H)
    M = _mask(rng, N, D)
    Yg = np.where(M, Y, np.nan)
    p_in = {k: np.array(v, copy=True) for k, v in p.items()}
    want_y, want_l = MR.enumerate_all(_ref_kind(kind), p, Yg, M)
    got_y = m.reconstruct(p, {"y": Yg, "mask": M})
    got_l = m.log_likelihood(p, {"y": Yg, "mask": M}, per_datapoint=True)
    for k in p_in:
        np.testing.assert_array_equal(p[k], p_in[k])
    assert np.isfinite(got_y).all() and np.isfinite(got_l).all()
    _check_rows(kind + " enumeration", got_y, want_y)
    _check_ll(kind + " enumeration", got_l, want_l, M, p, H)
    tot = m.log_likelihood(p, {"y": Yg, "mask": M})
    np.testing.assert_allclose(tot, got_l.sum(), rtol=1e-12)


# --------------------------------------------------------------------------------------------------------- 2: truncated
# One case per instantiation and branch of the launchers (dispatch is a function of H, D and H' alone, so the shape names
# the branch; test -> branch in DESIGN 4.16):
#   bsc_masked_estep_kernel<VPL>      H = 24 / 65 (first latent of the second slot) / 130 / 257 / 520 / 1024 (PM_MAX_H):
#                                     VPL 1, 2, 4, 8, 16, 16; H' = 12 and 16 give 66 and 120 candidate pairs: the second
#                                     pair a lane owns (own1 / a1 / pi_[1])
#   mca_masked_estep_kernel<DPL>      D = 64 / 70, 128 / 129, 200, 256 / 257, 512 / 513, 1024: DPL 1 / 2, 2 / 4, 4, 4 / 8,
#                                     8 / 16, 16 -- each full last slab (D = 64 DPL) once; H' = 12 and 16; the largest
#                                     dynamic LDS request (D = 1024, H' = 16: one wavefront per workgroup)
#   mca_masked_select_scores_kernel   H = 65, 70 (two H tiles), 130 (three), none a multiple of 64
#   recon_mca_kernel<DPL>             the same D buckets, from masked log-joints
TRUNC = ([(k, 70, 24, 6, 3, 130) for k in KINDS] +
         [("mca", 1024, 24, 6, 3, 24), ("mca", 1, 8, 4, 2, 24), ("mmca", 1024, 12, 5, 2, 16)] +
         [(k, D, H, Hp, g, 64) for k in ("bsc", "bsc_mu")
          for D, H, Hp, g in ((33, 65, 6, 3), (70, 130, 12, 3), (33, 257, 6, 3), (24, 520, 5, 2), (40, 1024, 16, 2))] +
         [(k, D, H, Hp, g, 64) for k in ("mca", "mmca")
          for D, H, Hp, g in ((129, 24, 6, 3), (200, 70, 12, 2), (257, 65, 5, 2), (513, 130, 6, 3), (1024, 20, 16, 2))] +
         [("mca", 64, 24, 6, 3, 64), ("mmca", 128, 24, 6, 3, 64), ("mca", 256, 24, 5, 2, 64), ("mmca", 512, 20, 5, 2, 64)])
GAP = 1e-9


def _entries(m):
    """The model's launch hook, wrapped to keep the names of the entry points that ran."""
    calls = []
    orig = m._call
    m._call = lambda label, entry, *args: (calls.append(entry), orig(label, entry, *args))[1]
    return calls


def _masked_entries(kind):
    if kind.startswith("bsc"):
        return {"pm_masked_prepare_f64", "pm_bsc_masked_estep_f64", "pm_recon_expect_f64"}
    sel = {"pm_mca_masked_select_scores_f64"} if kind == "mca" else set()
    return sel | {"pm_masked_prepare_f64", "pm_mca_masked_estep_f64", "pm_recon_expect_f64", "pm_recon_mca_f64"}


@pytest.mark.parametrize("kind,D,H,Hp,g,N", TRUNC)
def test_truncated_candidates_and_sums(dev, kind, D, H, Hp, g, N):
    rng = np.random.RandomState(D + H + KINDS.index(kind))
    m, p, Y = _problem(kind, rng, D, H, N, Hp, g)
    M = _mask(rng, N, D)
    Yg = np.where(M, Y, 1e300)
    # candidate lists are compared exactly: that says something only where the reference's own scores at the selection
    # boundary (the H'-th and (H'+1)-th) are further apart than two f64 evaluations of them can differ -- asserted on the
    # reference, for every row with an observed value (the unobserved row has its index rule below)
    sc, largest = MR.model_scores(_ref_kind(kind), p, Yg, M)
    gap = MR.boundary_gap(sc, Hp, largest)[M.any(axis=1)]              # (D = 1: half of the rows are unobserved)
    print("masked selection %-28s smallest boundary gap %.3e (needs > %.1e)" % ("%s D=%d H=%d H'=%d" % (kind, D, H, Hp),
                                                                               gap.min(), GAP))
    # (D = 1: a score is ONE term, max(w - y, 0) or b / sqrt(g), with nothing to sum -- both sides hold the same bits, zeros
    # tie exactly and the index rule decides them on both sides)
    assert gap.size == (N - 1 if D > 1 else M.any(axis=1).sum()) and ((gap > GAP).all() or D == 1), gap.min()
    kept = _capture(m)
    calls = _entries(m)
    got_y = m.reconstruct(p, {"y": Yg, "mask": M})
    assert _masked_entries(kind) <= set(calls), calls
    cand = kept["out"]["cand"].cpu().numpy()
    _, select = MR.model_terms(_ref_kind(kind), p)
    want_c = select(Yg, M, Hp)
    assert cand.shape == (N, Hp)
    np.testing.assert_array_equal(cand, want_c)
    if kind.startswith("bsc"):
        np.testing.assert_array_equal(cand[1], np.arange(H - Hp, H))      # nothing observed: the H' largest indices
    want_y, want_l = MR.from_candidates(_ref_kind(kind), p, Yg, M, cand, m.state_matrix)
    tag = "%s D=%d H=%d H'=%d" % (kind, D, H, Hp)
    _check_rows(tag, got_y, want_y)
    del calls[:]
    got_l = m.log_likelihood(p, {"y": Yg, "mask": M}, per_datapoint=True)
    assert (_masked_entries(kind) - {"pm_recon_expect_f64", "pm_recon_mca_f64"}) <= set(calls), calls
    np.testing.assert_array_equal(kept["out"]["cand"].cpu().numpy(), cand)
    _check_ll(tag, got_l, want_l, np.ones_like(M), p, H)      # (a truncated set's prior mass is below 1: no computed zero)


# ------------------------------------------------------------------------------- 2b: second trip of the grid-stride loops
# masked kernels: at most 2048 workgroups of four rows (grid_for_rows), so row 8192 is the first of a second trip; the recon
# kernels that consume the masked log-joints: 8192 workgroups, row 32768
@pytest.mark.parametrize("kind,N", [("bsc", 8192 + 77), ("mca", 8192 + 77), ("mca", 32768 + 77)])
def test_second_trip_of_the_row_loops(dev, kind, N):
    """Every per-wavefront LDS area (s_c / s_ac / s_gc, s_wr / s_e) is used again after the trailing wave_lds_sync().  The
    rows from 150 before each boundary onwards against the NumPy sums over the device's candidates; the whole result bit
    for bit against the same calls on shards of 4096 rows (a row's bits depend on that row alone)."""
    D, H, Hp, g = 8, 6, 4, 2
    rng = np.random.RandomState(N % 1000 + KINDS.index(kind))
    m, p, Y = _problem(kind, rng, D, H, N, Hp, g)
    M = _mask(rng, N, D)
    Yg = np.where(M, Y, np.nan)
    kept = _capture(m)
    got_y = m.reconstruct(p, {"y": Yg, "mask": M})
    cand = kept["out"]["cand"].cpu().numpy()
    got_l = m.log_likelihood(p, {"y": Yg, "mask": M}, per_datapoint=True)
    assert got_y.shape == (N, D) and np.isfinite(got_y).all() and np.isfinite(got_l).all()
    rows = np.concatenate([np.arange(b - 150, min(b + 227, N)) for b in (8192, 32768) if b < N])
    _, select = MR.model_terms(_ref_kind(kind), p)
    np.testing.assert_array_equal(cand[rows], select(Yg[rows], M[rows], Hp))
    want_y, want_l = MR.from_candidates(_ref_kind(kind), p, Yg[rows], M[rows], cand[rows], m.state_matrix)
    _check_rows("%s N=%d second trip" % (kind, N), got_y[rows], want_y)
    _check_ll("%s N=%d second trip" % (kind, N), got_l[rows], want_l, np.ones_like(M[rows]), p, H)
    parts = [(m.reconstruct(p, {"y": Yg[i:i + 4096], "mask": M[i:i + 4096]}),
              m.log_likelihood(p, {"y": Yg[i:i + 4096], "mask": M[i:i + 4096]}, per_datapoint=True)) for i in range(0, N, 4096)]
    _same_bits(np.concatenate([a for a, _ in parts]), got_y, "reconstruct in shards")
    _same_bits(np.concatenate([b for _, b in parts]), got_l, "log_likelihood in shards")


# ------------------------------------------------------------------------------------------------------------ 2c: limits
# (AT the limits -- H = PM_MAX_H = 1024 with H' = PM_MAX_HPRIME = 16, D = 1024 with H' = 16 -- are cases of TRUNC above)
@pytest.mark.parametrize("kind,D,H,Hp", [("bsc", 16, 1025, 4), ("bsc", 16, 40, 17), ("mca", 1025, 12, 4), ("mca", 16, 40, 17),
                                          ("mmca", 1025, 12, 4)])
def test_one_past_a_limit_raises(dev, kind, D, H, Hp):
    """HipError -- the library's PM_ERANGE or the host's own range check (some in the constructor) -- and no result."""
    from prosper_amd import _lib
    rng = np.random.RandomState(D + H + Hp)
    N = 12
    with pytest.raises(_lib.HipError):
        m, p, Y = _problem(kind, rng, D, H, N, Hp, 2)
        M = _mask(rng, N, D)
        m.reconstruct(p, {"y": Y, "mask": M})
    with pytest.raises(_lib.HipError):
        m, p, Y = _problem(kind, rng, D, H, N, Hp, 2)
        m.log_likelihood(p, {"y": Y, "mask": _mask(rng, N, D)}, per_datapoint=True)


# --------------------------------------------------------------------------------------------------------- 3: sub-model
# (BSC with mu at H' = gamma = H: the unmasked selection ranks the UNCENTRED <W_h, y> / |W_h| -- the reference's own rule,
# bsc_et.py:98-115 -- while the masked one ranks b_h = <W_h, y - mu>_obs as DESIGN 4.16 defines it; on a truncated state set
# the two pick different candidates for some rows, so the sub-model comparison holds only where the set is complete)
SUB = {"bsc": (70, 24, 6, 3), "bsc_mu": (70, 8, 8, 8), "mca": (70, 24, 6, 3), "mmca": (70, 24, 6, 3)}


@pytest.mark.parametrize("kind", KINDS)
def test_shared_mask_equals_the_unmasked_sub_model(dev, kind):
    """One mask for all rows: the existing, trusted unmasked path on W[obs], y[:, obs] is the reference."""
    (D, H, Hp, g), N = SUB[kind], 130
    rng = np.random.RandomState(40 + KINDS.index(kind))
    m, p, Y = _problem(kind, rng, D, H, N, Hp, g)
    obs = rng.uniform(size=D) < 0.5
    M = np.tile(obs, (N, 1))
    Yg = np.where(M, Y, -np.inf)
    sub = type(m)(int(obs.sum()), H, Hp, g)
    ps = dict(p, W=p["W"][obs])
    if "mu" in p:
        ps["mu"] = p["mu"][obs]
    want_y = sub.reconstruct(ps, {"y": Y[:, obs]})
    want_l = sub.log_likelihood(ps, {"y": Y[:, obs]}, per_datapoint=True)
    got_y = m.reconstruct(p, {"y": Yg, "mask": M})
    got_l = m.log_likelihood(p, {"y": Yg, "mask": M}, per_datapoint=True)
    _check_rows(kind + " sub-model", got_y[:, obs], want_y)
    np.testing.assert_allclose(got_l, want_l, rtol=RTOL)
    np.testing.assert_allclose(m.log_likelihood(p, {"y": Yg, "mask": M}), sub.log_likelihood(ps, {"y": Y[:, obs]}), rtol=RTOL)
    # an all-ones mask against no mask
    ones = np.ones((N, D), dtype=np.uint8)
    _check_rows(kind + " all-ones", m.reconstruct(p, {"y": Y, "mask": ones}), m.reconstruct(p, {"y": Y}))
    np.testing.assert_allclose(m.log_likelihood(p, {"y": Y, "mask": ones}, per_datapoint=True),
                               m.log_likelihood(p, {"y": Y}, per_datapoint=True), rtol=RTOL)


# ----------------------------------------------------------------------------------------------- 4: garbage invariance
@pytest.mark.parametrize("kind", KINDS)
def test_unobserved_entries_change_no_bit(dev, kind):
    D, H, Hp, g, N = 23, 12, 5, 3, 90
    rng = np.random.RandomState(60 + KINDS.index(kind))
    m, p, Y = _problem(kind, rng, D, H, N, Hp, g)
    M = _mask(rng, N, D)
    base_y = m.reconstruct(p, {"y": np.where(M, Y, 0.0), "mask": M})
    base_l = m.log_likelihood(p, {"y": np.where(M, Y, 0.0), "mask": M}, per_datapoint=True)
    base_t = m.log_likelihood(p, {"y": np.where(M, Y, 0.0), "mask": M})
    assert np.isfinite(base_y).all() and np.isfinite(base_l).all()
    for fill in (np.nan, np.inf, 1e300):
        Yg = np.where(M, Y, fill)
        _same_bits(m.reconstruct(p, {"y": Yg, "mask": M}), base_y, "reconstruct, fill %r" % fill)
        _same_bits(m.log_likelihood(p, {"y": Yg, "mask": M}, per_datapoint=True), base_l, "rows, fill %r" % fill)
        assert m.log_likelihood(p, {"y": Yg, "mask": M}) == base_t
    # a NaN at an OBSERVED entry: that row is NaN and no other row moves
    n = 7
    d = int(np.nonzero(M[n])[0][0])
    Yn = np.where(M, Y, np.nan)
    Yn[n, d] = np.nan
    rows = m.reconstruct(p, {"y": Yn, "mask": M})
    ll = m.log_likelihood(p, {"y": Yn, "mask": M}, per_datapoint=True)
    assert np.isnan(rows[n]).all() and np.isnan(ll[n])
    _same_bits(np.delete(rows, n, axis=0), np.delete(base_y, n, axis=0), "other rows")
    _same_bits(np.delete(ll, n), np.delete(base_l, n), "other rows' log-likelihood")


# ---------------------------------------------------------------------------------------------------------------- 5: bits
@pytest.mark.parametrize("kind", KINDS)
def test_bits_repeat_across_calls_builds_row_order_shards_and_mask_types(dev, kind):
    import torch
    from prosper_amd.em.camodels._device import DeviceArray
    D, H, Hp, g, N = 24, 12, 5, 3, 700
    rng = np.random.RandomState(80 + KINDS.index(kind))
    m, p, Y = _problem(kind, rng, D, H, N, Hp, g)
    M = _mask(rng, N, D)
    a = m.reconstruct(p, {"y": Y, "mask": M})
    l = m.log_likelihood(p, {"y": Y, "mask": M}, per_datapoint=True)
    t = m.log_likelihood(p, {"y": Y, "mask": M})
    _same_bits(m.reconstruct(p, {"y": Y, "mask": M}), a, "second call")
    _same_bits(m.log_likelihood(p, {"y": Y, "mask": M}, per_datapoint=True), l, "second call")
    d = m.reconstruct(p, {"y": Y, "mask": M}, device=True)
    assert isinstance(d, DeviceArray) and d.tensor.is_cuda
    _same_bits(np.asarray(d), a, "device output")
    m.deterministic = True
    _same_bits(m.reconstruct(p, {"y": Y, "mask": M}), a, "deterministic build")
    _same_bits(m.log_likelihood(p, {"y": Y, "mask": M}, per_datapoint=True), l, "deterministic build")
    assert m.log_likelihood(p, {"y": Y, "mask": M}) == t
    m.deterministic = False
    perm = rng.permutation(N)
    _same_bits(m.reconstruct(p, {"y": Y[perm], "mask": M[perm]}), a[perm], "row permutation")
    _same_bits(m.log_likelihood(p, {"y": Y[perm], "mask": M[perm]}, per_datapoint=True), l[perm], "row permutation")
    _same_bits(m.reconstruct(p, {"y": Y[130:333], "mask": M[130:333]}), a[130:333], "shard")
    _same_bits(m.log_likelihood(p, {"y": Y[130:333], "mask": M[130:333]}, per_datapoint=True), l[130:333], "shard")
    _same_bits(m.reconstruct(p, {"y": Y[5:6], "mask": M[5:6]}), a[5:6], "one row")
    # the mask's types: bool, uint8, any numeric; NumPy, torch (host and device, used in place), DeviceArray; strided
    wide = torch.zeros((N, D + 9), dtype=torch.uint8, device=dev)
    wide[:, :D] = torch.from_numpy(M.astype(np.uint8) * 200).to(dev)
    for what, mk in (("uint8", M.astype(np.uint8)), ("float", M * 2.5), ("int64", -M.astype(np.int64)),
                     ("torch host bool", torch.from_numpy(M)), ("torch device uint8", torch.from_numpy(M.astype(np.uint8)).to(dev)),
                     ("device view with its own leading dimension", wide[:, :D]),
                     ("DeviceArray", DeviceArray(torch.from_numpy(M).to(dev))),
                     ("torch device float", torch.from_numpy(M * 1.0).to(dev))):
        _same_bits(m.reconstruct(p, {"y": Y, "mask": mk}), a, what)
    # calls without the key run none of the new entries
    calls = []
    orig = m._call
    m._call = lambda label, entry, *args: (calls.append(entry), orig(label, entry, *args))[1]
    m.reconstruct(p, {"y": Y})
    m.log_likelihood(p, {"y": Y})
    assert calls and not [c for c in calls if "masked" in c], calls
    del calls[:]
    m.reconstruct(p, {"y": Y, "mask": M})
    assert [c for c in calls if "masked" in c] and "pm_gemm_nt_rows_f64" in calls, calls
    assert not [c for c in calls if c in ("pm_gemm_nt_f64", "pm_gemm_nt_small_f64")], calls


# ------------------------------------------------------------------------------------------- 6: training undisturbed
def _schedule(steps):
    from prosper_amd.em.annealing import LinearAnnealing
    a = LinearAnnealing(steps)
    a["T"] = [(0, 2.), (.7, 1.)]
    a["Ncut_factor"] = [(0, 0.), (2. / 3, 1.)]
    a["anneal_prior"] = False
    a.as_dict = lambda: {k: a[k] for k in ("T", "Ncut_factor")}
    return a


def _train(m, params, Y, Yh, Mh, steps, interleave):
    a = _schedule(steps)
    for _ in range(steps):
        params = m.step(a, params, {"y": Y})
        if interleave:
            hp = (m.Hprime, m.gamma)
            q = {k: np.array(v, copy=True) for k, v in params.items()}
            out = m.reconstruct(q, {"y": Yh, "mask": Mh})
            ll = m.log_likelihood(q, {"y": Yh, "mask": Mh})
            assert out.shape == Yh.shape and np.isfinite(out).all() and np.isfinite(ll)
            assert (m.Hprime, m.gamma) == hp
        a.next()
    return {k: np.array(v, copy=True) for k, v in params.items()}, getattr(m, "spec_hits", None)


@pytest.mark.parametrize("kind", ["bsc", "mca", "mmca"])
def test_training_undisturbed(dev, kind):
    rng = np.random.RandomState(14)
    D, H, N, Nh = 20, 10, 900, 200
    _, p, Y = _problem(kind, rng, D, H, N + Nh, 5, 3)
    p = dict(p, W=p["W"] * rng.uniform(0.9, 1.1, size=p["W"].shape))
    Yt, Yh = Y[:N], Y[N:]
    Mh = _mask(rng, Nh, D)

    def det():
        m = _problem(kind, np.random.RandomState(0), D, H, 4, 5, 3)[0]
        m.deterministic = True
        return m
    ref, hits_ref = _train(det(), {k: np.array(v, copy=True) for k, v in p.items()}, Yt, Yh, Mh, 5, False)
    got, hits_got = _train(det(), {k: np.array(v, copy=True) for k, v in p.items()}, Yt, Yh, Mh, 5, True)
    for k in ref:
        np.testing.assert_array_equal(ref[k], got[k], err_msg=k)
    if kind == "bsc":
        assert hits_ref is not None and hits_ref == hits_got, (hits_ref, hits_got)


# ---------------------------------------------------------------------------------------------------------------- 7: image
A_BAR, SIGMA, PI, PB = 3.0, 1.0, 0.2, 4


def _bars_problem(kind, seed):
    """The 40 x 37 bars image of tests/test_patches_gpu.py at its generating parameters, H' = gamma = H = 8, 30 % missing."""
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    from prosper_amd.em.camodels.mca_et import MCA_ET
    rng = np.random.RandomState(seed)
    clean, noisy, _, _ = P.bars_image(rng, 40, 37, A_BAR, PI, SIGMA, mca=kind == "mca")
    W = P.bars_W(PB, A_BAR)
    H = 2 * PB
    if kind == "mca":
        W = np.where(W < 0.05, 0.05, W)              # as check_params does
    mask = rng.uniform(size=clean.shape) >= 0.3
    model = (MCA_ET if kind == "mca" else BSC_ET)(PB * PB, H, H, H)
    return model, {"W": W, "pi": PI, "sigma": SIGMA}, clean, noisy, mask


@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("kind", ["bsc", "mca"])
def test_image_composition_enumeration_and_inpainting(dev, kind, stride):
    from prosper_amd.utils import patches as U
    m, p, clean, noisy, mask = _bars_problem(kind, 0)
    holes = np.where(mask, noisy, np.nan)
    got = m.reconstruct_image(p, holes, mask=mask, stride=stride)
    assert got.shape == noisy.shape and got.dtype == np.float64 and np.isfinite(got).all()
    # (a) the composition, bit for bit, for two chunk sizes and both builds
    Yp, _ = U.extract_patches(holes, PB, stride)
    Mp, _ = U.extract_patches(mask.astype(np.float64), PB, stride)
    comp = U.average_patches(m.reconstruct(p, {"y": Yp, "mask": Mp}), noisy.shape, PB, stride)
    _same_bits(got, comp, "composition")
    nc = len(P.starts(37, PB, stride))
    for chunk in (nc, 7 * nc + 3):
        _same_bits(U.denoise_image(m, p, holes, stride=stride, chunk=chunk, mask=mask), got, "chunk %d" % chunk)
    _same_bits(m.reconstruct_image(p, np.where(mask, noisy, 1e300), mask=mask.astype(np.uint8), stride=stride), got, "fill")
    m.deterministic = True
    try:
        _same_bits(m.reconstruct_image(p, holes, mask=mask, stride=stride, chunk=5 * nc), got, "deterministic build")
    finally:
        m.deterministic = False
    # (b) against the enumeration of every patch's masked posterior mean, averaged
    rows, _ = MR.enumerate_all(kind, p, P.extract(holes, (PB, PB), stride), P.extract(mask, (PB, PB), stride) != 0)
    want = P.average(rows, noisy.shape, (PB, PB), stride)
    err = np.abs(got - want).max() / np.abs(want).max()
    print("masked reconstruct_image %s stride %d against enumeration: %.3e of max |image| (bound 1e-11)" % (kind, stride, err))
    assert err <= 1e-11, err
    # (c) inpainting inpaints, denoising denoises: first on the NumPy reference (a failure there blames the inputs)
    fill = noisy[mask].mean()
    mse_fill = float(((fill - clean[~mask]) ** 2).mean())
    mse_noisy = float(((noisy[mask] - clean[mask]) ** 2).mean())
    for what, img in (("numpy", want), ("device", got)):
        mse_mis, mse_obs = float(((img - clean)[~mask] ** 2).mean()), float(((img - clean)[mask] ** 2).mean())
        print("bars %s stride %d (%s): missing pixels MSE %.4f (mean fill %.4f), observed pixels MSE %.4f (noisy %.4f)" % (
            kind, stride, what, mse_mis, mse_fill, mse_obs, mse_noisy))
        assert mse_mis < mse_fill and mse_obs < mse_noisy, what


# ------------------------------------------------------------------------------------------------------------ 8: refusals
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
    Y, M = rng.normal(size=(N, D)), rng.uniform(size=(N, D)) < 0.5
    p = {"W": rng.normal(size=(D, H)), "pi": 0.2, "sigma": 1.0}
    for m in (DSC_ET(D, H, 4, 2), TSC_ET(D, H, 4, 2), GSC(D, H, 4, 2), MoG(D, H), MoP(D, H)):
        calls = []
        if hasattr(m, "_call"):
            orig = m._call
            m._call = lambda label, entry, *args, _o=orig: (calls.append(entry), _o(label, entry, *args))[1]
        for call in (lambda: m.reconstruct(p, {"y": Y, "mask": M}), lambda: m.log_likelihood(p, {"y": Y, "mask": M}),
                     lambda: m.reconstruct_image(p, rng.normal(size=(9, 9)), mask=np.ones((9, 9)), patch=4)):
            with pytest.raises(NotImplementedError, match=type(m).__name__):
                call()
        assert not calls, (type(m).__name__, calls)
    m = BSC_ET(D, H, 4, 2)
    with pytest.raises(NotImplementedError, match="exact"):
        m.log_likelihood(p, {"y": Y, "mask": M}, exact=True)
    with pytest.raises(ValueError, match="center"):
        m.reconstruct_image(p, rng.normal(size=(9, 9)), mask=np.ones((9, 9)), center=True)
    with pytest.raises(ValueError, match="mask"):
        m.reconstruct_image(p, rng.normal(size=(9, 9)), mask=np.ones((9, 8)))
    for bad in (M[:, :-1], M[:-1], M.ravel(), M[:, :, None]):
        with pytest.raises(ValueError, match="mask"):
            m.reconstruct(p, {"y": Y, "mask": bad})
        with pytest.raises(ValueError, match="mask"):
            m.log_likelihood(p, {"y": Y, "mask": bad})
    big = BSC_ET(D, 20, 17, 2)
    with pytest.raises(_lib.HipError, match="16"):
        big.reconstruct({"W": rng.normal(size=(D, 20)), "pi": 0.1, "sigma": 1.0}, {"y": Y, "mask": M})
    # the model still works afterwards
    assert np.isfinite(m.reconstruct(p, {"y": Y, "mask": M})).all()
