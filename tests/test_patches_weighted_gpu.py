"""The weighted overlap average on the device.  First the two C entries by themselves, bit for bit against the
NumPy statement (tests/patches_weighted_reference.py, pinned on the CPU by tests/test_patches_weighted_cpu.py): every weight
form, with and without means, leading dimensions past D, running sums that do not start at zero, ranges cut inside a patch
row, den = NULL, both library builds, 0 / 0, NaN estimates and negative variances.  Then ``denoise_image(aggregate=
'precision')`` against the same loops applied to what ``reconstruct(variance=True)`` returned for the same patches.

Every comparison is bit equality: both sides run the same IEEE operations in the same order (one rounded product, one
rounded addition per patch, one division per pixel).  The only inequality is "the precision aggregate denoises"."""
import functools

import numpy as np
import pytest

import patches_reference as P
import patches_weighted_reference as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _same_bits(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.float64, (what, got.shape, want.shape, got.dtype)
    diff = _bits(got) != _bits(want)
    assert not diff.any(), "%s: %d of %d values differ, first at %s" % (what, diff.sum(), diff.size, np.argwhere(diff)[:1])


def _pair(patch):
    return (patch, patch) if isinstance(patch, int) else tuple(patch)


# (image shape, patch, stride): the geometries of tests/test_patches_gpu.py's SWEEP -- odd sizes, strides that do not divide,
# rectangular patches, p = image, a stack, images wider and taller than one tile, a patch of more values than one staging
# holds -- and D = 4096 (21 patches), where the staging holds one patch at a time and its two rows pass 48 KiB of LDS
GEOMETRIES = [((9, 11), 4, 1), ((13, 17), (3, 5), 2), ((21, 19), 4, 3), ((8, 8), 8, 1), ((7, 9), (7, 9), 4),
              ((3, 10, 9), (4, 3), 3), ((15, 14), 5, 2), ((2, 9, 12), 2, 1), ((70, 150), 4, 1), ((41, 133), (8, 8), 5),
              ((37, 45), 16, 1), ((40, 200), (2, 40), 2), ((5, 6), 1, 1), ((66, 70), 64, 1)]
FORMS = ["wgt0", "wgt1", "window", "both"]
FLOOR = 0.37
PAD_E, PAD_W = 3, 5                                  # lde = D + 3, ldw = D + 5


def _full(shape):
    return (1,) + tuple(shape) if len(shape) == 2 else tuple(shape)


@functools.lru_cache(maxsize=None)
def _case(gi, form, with_means):
    """The inputs of one case and the reference's (num, den) from non-zero running sums.  Computed once, never changed."""
    shape, patch, stride = GEOMETRIES[gi]
    ph, pw = _pair(patch)
    rng = np.random.RandomState(1000 + 10 * gi + FORMS.index(form))
    N, D = len(P.grid(shape, (ph, pw), stride)), ph * pw
    E = rng.normal(size=(N, D)) * 10.0 ** rng.randint(-2, 3, size=(N, 1))
    mu = rng.normal(size=N) * 3 if with_means else None
    wgt, wmode, window = None, 0, None
    if form == "wgt0":
        wgt = rng.uniform(0.1, 2.0, size=(N, D)) * 10.0 ** rng.randint(-1, 2, size=(N, 1))
    elif form in ("wgt1", "both"):
        wgt, wmode = rng.uniform(-0.2, 2.0, size=(N, D)), 1                # variances: some negative, some exactly 0
        wgt[rng.uniform(size=(N, D)) < 0.05] = 0.0
    if form in ("window", "both"):
        window = rng.uniform(0.25, 1.5, size=D)
    num0, den0 = rng.normal(size=_full(shape)), rng.uniform(0.5, 1.5, size=_full(shape))
    num, den = W.accumulate(num0.copy(), den0.copy(), E, shape, (ph, pw), stride, wgt, wmode, FLOOR, window, mu)
    out = dict(shape=shape, patch=(ph, pw), stride=stride, N=N, D=D, E=E, mu=mu, wgt=wgt, wmode=wmode, window=window,
               num0=num0, den0=den0, num=num, den=den)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _padded(a, pad, dev):
    """(device tensor (N, D + pad) holding ``a`` with NaN in the padding, its leading dimension), or (None, 0)."""
    import torch
    if a is None:
        return None, 0
    t = torch.full((a.shape[0], a.shape[1] + pad), float("nan"), dtype=torch.float64, device=dev)
    t[:, :a.shape[1]] = torch.from_numpy(np.array(a)).to(dev)
    return t, a.shape[1] + pad


def _to(a, dev):
    import torch
    return None if a is None else torch.from_numpy(np.array(a)).to(dev)


def _run(c, dev, det=False, cuts=None, with_den=True, wgt=None):
    """The entry on case ``c`` from its non-zero running sums, in the ranges ``cuts`` (default: one call); (num, den)."""
    from prosper_amd.utils import patches as U
    geo = U._geometry(c["shape"], c["patch"], c["stride"])
    est, lde = _padded(c["E"], PAD_E, dev)
    wg, ldw = _padded(c["wgt"] if wgt is None else wgt, PAD_W, dev)
    win, mu = _to(c["window"], dev), _to(c["mu"], dev)
    num, den = _to(c["num0"], dev), _to(c["den0"], dev)
    cuts = cuts or [0, c["N"]]
    for a, b in zip(cuts, cuts[1:]):
        U._accumulate_w(num, den if with_den else None, est[a:], lde, None if wg is None else wg[a:], ldw, c["wmode"], FLOOR,
                        win, None if mu is None else mu[a:], geo, a, b - a, det)
    return num, den


# ------------------------------------------------------------------------------------------------- the entries by themselves
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("gi", range(len(GEOMETRIES)))
def test_accumulate_and_finish_equal_the_reference_bit_for_bit(dev, gi, form):
    from prosper_amd.utils import patches as U
    for with_means in (False, True):
        c = _case(gi, form, with_means)
        num, den = _run(c, dev)
        what = "%s %s means=%s" % (GEOMETRIES[gi], form, with_means)
        _same_bits(num.cpu().numpy(), c["num"], "num " + what)
        _same_bits(den.cpu().numpy(), c["den"], "den " + what)
        geo = U._geometry(c["shape"], c["patch"], c["stride"])
        out = U._finish_w(num, den, geo, False)
        _same_bits(out.cpu().numpy(), W.finish(c["num"], c["den"]), "finish " + what)
        # out may alias num
        U._lib.call("pm_patches_finish_w_f64", U._ptr(num), U._ptr(den), geo[0][2], U._ptr(num), geo[0][2], *geo[0],
                    U._stream(dev))
        _same_bits(num.cpu().numpy(), out.cpu().numpy(), "finish in place " + what)


@pytest.mark.parametrize("gi", range(len(GEOMETRIES)))
def test_ranges_den_null_and_both_builds(dev, gi):
    """Ranges that start and end inside patch rows give the bits of one range; den = NULL leaves num's bits and does not
    touch den; the deterministic build gives the same bits."""
    c = _case(gi, "both", True)
    N = c["N"]
    cuts = sorted(set([0, N // 5, N // 5 + 1, N // 2, N - 1, N]))
    num, den = _run(c, dev, cuts=cuts)
    _same_bits(num.cpu().numpy(), c["num"], "num in ranges %s" % cuts)
    _same_bits(den.cpu().numpy(), c["den"], "den in ranges %s" % cuts)
    num, den = _run(c, dev, with_den=False)
    _same_bits(num.cpu().numpy(), c["num"], "num with den = NULL")
    _same_bits(den.cpu().numpy(), c["den0"], "den untouched")
    num, den = _run(c, dev, det=True, cuts=cuts)
    _same_bits(num.cpu().numpy(), c["num"], "num, deterministic build")
    _same_bits(den.cpu().numpy(), c["den"], "den, deterministic build")


@pytest.mark.parametrize("gi", range(len(GEOMETRIES)))
def test_without_weights_it_is_the_plain_accumulate(dev, gi):
    import torch
    from prosper_amd.utils import patches as U
    c = _case(gi, "window", True)
    geo = U._geometry(c["shape"], c["patch"], c["stride"])
    est, lde = _padded(c["E"], PAD_E, dev)
    mu = _to(c["mu"], dev)
    for means in (None, mu):
        plain = _to(c["num0"], dev)
        U._accumulate(plain, est, lde, means, geo, 0, c["N"], False)
        num, den = _to(c["num0"], dev), torch.zeros(_full(c["shape"]), dtype=torch.float64, device=dev)
        U._accumulate_w(num, den, est, lde, None, 0, 0, 0.0, None, means, geo, 0, c["N"], False)
        _same_bits(num.cpu().numpy(), plain.cpu().numpy(), "num against pm_patches_accumulate_f64")
        _same_bits(den.cpu().numpy(), P.cover(c["shape"], c["patch"], c["stride"]).astype(np.float64), "den = cover count")


def test_a_negative_variance_counts_as_zero(dev):
    for gi in (2, 5, 9):
        c = _case(gi, "wgt1", True)
        assert (c["wgt"] < 0).any()
        num, den = _run(c, dev, wgt=np.where(c["wgt"] < 0, 0.0, c["wgt"]))
        _same_bits(num.cpu().numpy(), c["num"])
        _same_bits(den.cpu().numpy(), c["den"])


@pytest.mark.parametrize("shape,patch,stride", [((21, 19), (4, 4), 3), ((3, 10, 9), (4, 3), 3), ((40, 70), (8, 8), 1)])
def test_zero_weights_and_nan_estimates(dev, shape, patch, stride):
    """A pixel all of whose weights are 0 is NaN (0 / 0) and no other pixel is; a NaN estimate row makes NaN exactly the
    pixels of its patch and changes no other pixel's bits."""
    from prosper_amd.utils import patches as U
    rng = np.random.RandomState(sum(shape))
    g = P.grid(shape, patch, stride)
    N, D = len(g), patch[0] * patch[1]
    full = _full(shape)
    E = rng.normal(size=(N, D))
    wgt = rng.uniform(0.5, 2.0, size=(N, D))
    window = rng.uniform(0.5, 1.5, size=patch)
    clean = U.average_patches(E, shape, patch, stride, weights=wgt, window=window)
    _same_bits(clean, W.average(E, shape, patch, stride, wgt=wgt, window=window), "average_patches(weights, window)")
    assert np.isfinite(clean).all()
    pixels = [(0, 0, 0), (full[0] - 1, full[1] - 1, full[2] - 1), (0, full[1] // 2, full[2] // 2)]
    w0 = wgt.copy()
    for k, (b, i, j) in enumerate(g):
        for (pb, pi, pj) in pixels:
            if b == pb and i <= pi < i + patch[0] and j <= pj < j + patch[1]:
                w0[k, (pi - i) * patch[1] + (pj - j)] = 0.0
    out = U.average_patches(E, shape, patch, stride, weights=w0, window=window).reshape(full)
    want = np.zeros(full, dtype=bool)
    for pix in pixels:
        want[pix] = True
    assert np.array_equal(np.isnan(out), want), (np.isnan(out).sum(), want.sum())
    _same_bits(out[~want], clean.reshape(full)[~want], "pixels with weights left")
    for k in (0, N // 2, N - 1):
        bad = E.copy()
        bad[k] = np.nan
        out = U.average_patches(bad, shape, patch, stride, weights=wgt, window=window).reshape(full)
        b, i, j = g[k]
        want = np.zeros(full, dtype=bool)
        want[b, i:i + patch[0], j:j + patch[1]] = True
        assert np.array_equal(np.isnan(out), want), (k, np.isnan(out).sum(), want.sum())
        _same_bits(out[~want], clean.reshape(full)[~want], "pixels outside the NaN patch")


# ------------------------------------------------------------------------------------------------------------- model level
PB = 4
MODELS = ["bsc", "mca", "mog_diagonal"]
IMAGES = {"image": (12, 13), "stack": (2, 9, 10)}


def _model(name, seed=7):
    """Tiny models at D = 16: BSC / MCA / GSC with H = 6, H' = 4, gamma = 2; MoG diagonal with H = 4."""
    from test_reconstruct_gpu import _mixture, _problem
    rng = np.random.RandomState(seed)
    if name.startswith("mo"):
        m, p, _, _ = _mixture(name, rng, 16, 4, 4)
    else:
        m, p, _, _, _ = _problem(name, rng, 16, 6, 4, 4, 2)
    return m, p


def _reference(m, p, img, stride, floor, center=False, mask=None, window=None, precision=True):
    """(image, var_map) by the reference loops on the (est, V) that reconstruct(variance=True) returns for the same patches."""
    from prosper_amd.utils import patches as U
    Y, means = U.extract_patches(img, PB, stride, center=center)
    data = {"y": Y}
    if mask is not None:
        data["mask"] = U.extract_patches(mask.astype(np.float64), PB, stride)[0] != 0
    est, V = m.reconstruct(p, data, variance=True)
    kw = dict(wgt=V, wmode=1, floor=floor) if precision else {}
    win = None if window is None else np.asarray(window, dtype=np.float64).reshape(-1)
    image = W.average(est, img.shape, (PB, PB), stride, window=win, means=means, **kw)
    return image, W.average(V, img.shape, (PB, PB), stride, window=win, **kw)


@pytest.mark.parametrize("which", sorted(IMAGES))
@pytest.mark.parametrize("name", MODELS)
def test_precision_aggregate_is_the_reference_on_reconstructs_output(dev, name, which):
    m, p = _model(name)
    rng = np.random.RandomState(3)
    img = rng.uniform(0.0, 3.0, size=IMAGES[which])
    nc = len(P.starts(img.shape[-1], PB, 1))
    f = 0.2
    want, want_var = _reference(m, p, img, 1, f)
    got = m.reconstruct_image(p, img, aggregate='precision', floor=f)
    assert np.isfinite(got).all() and got.shape == img.shape
    _same_bits(got, want, "%s precision" % name)
    got, var = m.reconstruct_image(p, img, aggregate='precision', floor=f, variance=True)
    _same_bits(got, want, "%s precision, variance=True: the image" % name)
    _same_bits(var, want_var, "%s var_map" % name)
    assert (var >= 0).all()
    # one patch row per chunk against the default, and the deterministic build
    got, var = m.reconstruct_image(p, img, aggregate='precision', floor=f, variance=True, chunk=nc)
    _same_bits(got, want, "%s chunk = one patch row" % name)
    _same_bits(var, want_var, "%s var_map, chunk = one patch row" % name)
    # center=True adds the patch mean to the estimate; a stride that does not divide
    want, want_var = _reference(m, p, img, 3, f, center=True)
    got, var = m.reconstruct_image(p, img, aggregate='precision', floor=f, variance=True, center=True, stride=3, chunk=2 * nc)
    _same_bits(got, want, "%s centred" % name)
    _same_bits(var, want_var, "%s centred var_map" % name)
    # a window, under both aggregates
    win = np.outer(np.hanning(PB + 2)[1:-1], np.hanning(PB + 2)[1:-1])
    want, want_var = _reference(m, p, img, 2, f, window=win)
    got, var = m.reconstruct_image(p, img, aggregate='precision', floor=f, variance=True, stride=2, window=win)
    _same_bits(got, want, "%s precision with a window" % name)
    _same_bits(var, want_var, "%s var_map with a window" % name)
    want, want_var = _reference(m, p, img, 2, f, window=win, precision=False)
    got, var = m.reconstruct_image(p, img, variance=True, stride=2, window=win.reshape(-1), chunk=nc)
    _same_bits(got, want, "%s mean with a window" % name)
    _same_bits(var, want_var, "%s var_map, mean with a window" % name)


@pytest.mark.parametrize("which", sorted(IMAGES))
def test_precision_aggregate_with_a_mask(dev, which):
    """BSC, 30 % of the pixels missing (NaN in the image): the masked reconstruct()'s (est, V) through the reference loops."""
    m, p = _model("bsc")
    rng = np.random.RandomState(4)
    img = rng.uniform(0.0, 3.0, size=IMAGES[which])
    mask = rng.uniform(size=img.shape) >= 0.3
    holes = np.where(mask, img, np.nan)
    nc = len(P.starts(img.shape[-1], PB, 1))
    want, want_var = _reference(m, p, holes, 1, 0.15, mask=mask)
    assert np.isfinite(want).all()
    got, var = m.reconstruct_image(p, holes, mask=mask, aggregate='precision', floor=0.15, variance=True)
    _same_bits(got, want, "masked precision")
    _same_bits(var, want_var, "masked var_map")
    got = m.reconstruct_image(p, holes, mask=mask, aggregate='precision', floor=0.15, chunk=nc)
    _same_bits(got, want, "masked precision, chunk = one patch row")


@pytest.mark.parametrize("name", ["bsc", "gsc_diagonal", "mog_diagonal"])
def test_default_floor_is_the_explicit_product(dev, name):
    from prosper_amd.utils import patches as U
    m, p = _model(name)
    if name == "bsc":
        nv = float(p["sigma"]) ** 2
    elif name == "gsc_diagonal":
        assert np.asarray(p["sigma_sq"]).shape == (16,)
        nv = float(np.mean(p["sigma_sq"]))
    else:
        assert np.asarray(p["sigmas_sq"]).shape == (4, 16)
        nv = float(np.mean(p["sigmas_sq"]))
    assert m._noise_variance(p) == nv
    rng = np.random.RandomState(5)
    img = rng.uniform(0.0, 3.0, size=(12, 13))
    got, var = m.reconstruct_image(p, img, aggregate='precision', variance=True)
    want, want_var = m.reconstruct_image(p, img, aggregate='precision', floor=U.PRECISION_FLOOR * nv, variance=True)
    _same_bits(got, want, "%s floor=None" % name)
    _same_bits(var, want_var, "%s floor=None, var_map" % name)
    _same_bits(got, _reference(m, p, img, 1, U.PRECISION_FLOOR * nv)[0], "%s floor=None against the reference" % name)


@pytest.mark.parametrize("name", MODELS)
def test_the_mean_aggregate_runs_todays_entries_and_gives_todays_bits(dev, name, monkeypatch):
    from prosper_amd import _lib
    from prosper_amd.utils import patches as U
    m, p = _model(name)
    rng = np.random.RandomState(6)
    img = rng.uniform(0.0, 3.0, size=(2, 9, 10))
    Y, means = U.extract_patches(img, PB, 2, center=True)
    est, V = m.reconstruct(p, {"y": Y}, variance=True)
    want = U.average_patches(est, img.shape, PB, 2, means=means)
    want_var = U.average_patches(V, img.shape, PB, 2)
    _same_bits(want, P.average(est, img.shape, (PB, PB), 2, means=means))
    names = []
    orig = _lib.call

    def spy(name_, *a, **k):
        names.append(name_)
        return orig(name_, *a, **k)
    monkeypatch.setattr(_lib, "call", spy)
    got = m.reconstruct_image(p, img, stride=2, center=True, aggregate='mean')
    got2, var = U.denoise_image(m, p, img, stride=2, center=True, variance=True, aggregate='mean', floor=0.5)
    patch_calls = [n for n in names if n.startswith("pm_patches_")]
    assert set(patch_calls) == {"pm_patches_extract_f64", "pm_patches_accumulate_f64", "pm_patches_finish_f64"}, set(patch_calls)
    assert not [n for n in names if "_w_f64" in n]
    _same_bits(got, want, "%s mean" % name)
    _same_bits(got2, want, "%s mean, variance=True" % name)
    _same_bits(var, want_var, "%s mean var_map" % name)
    # ... and the weighted entries are what the other aggregate runs
    del names[:]
    m.reconstruct_image(p, img, stride=2, aggregate='precision', floor=0.5)
    assert "pm_patches_accumulate_w_f64" in names and "pm_patches_finish_w_f64" in names
    assert "pm_patches_accumulate_f64" not in names and "pm_patches_finish_f64" not in names


@pytest.mark.parametrize("stride", [1, 3])
def test_the_precision_aggregate_inpaints_the_bars_image(dev, stride):
    """The bars image of test_denoising_denoises (BSC, seed 0) with 30 % of the pixels missing: the precision aggregate is
    closer to the clean image than the noisy one.  The difference to the mean aggregate is printed, not asserted."""
    from test_patches_gpu import _bars_problem
    m, p, clean, noisy = _bars_problem("bsc", 0)
    rng = np.random.RandomState(30)
    mask = rng.uniform(size=clean.shape) >= 0.3
    holes = np.where(mask, noisy, np.nan)
    mean = m.reconstruct_image(p, holes, mask=mask, stride=stride)
    prec = m.reconstruct_image(p, holes, mask=mask, stride=stride, aggregate='precision')
    mse = lambda a, sel=slice(None): float(((a - clean)[sel] ** 2).mean())
    print("bars bsc stride %d, 30 %% missing: MSE noisy %.4f, mean aggregate %.5f, precision aggregate %.5f (difference %+.3e; "
          "missing pixels only: %.5f against %.5f)" % (stride, mse(noisy), mse(mean), mse(prec), mse(prec) - mse(mean),
                                                       mse(mean, ~mask), mse(prec, ~mask)))
    assert np.isfinite(prec).all()
    assert mse(prec) < mse(noisy)
