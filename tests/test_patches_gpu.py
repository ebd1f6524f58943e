"""reconstruct_image() / utils.patches on the device, everything through the C ABI: patch extraction and the
overlap average bit for bit against the NumPy statement (tests/patches_reference.py, pinned on the CPU by
tests/test_patches_cpu.py), the composition with reconstruct() for all eight models, independence of the chunking, the
exact posterior mean by enumeration on a bars image, that denoising denoises, the plumbing apart from any model, NaN
pixels, an undisturbed training run and device-resident inputs and outputs.

Bounds: bit equality wherever both sides run the same IEEE operations in the same order; 1e-11 of the image's largest value
against NumPy enumeration (the project's bound for f64 against NumPy); the round-trip bounds count rounded
operations (k - 1 additions and one division for a pixel covered k times)."""
import math

import numpy as np
import pytest

import patches_reference as P
import recon_reference as R

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


# (image shape, patch, stride, dtype): odd sizes, strides that do not divide, rectangular patches, p = image, a stack,
# float32, images wider and taller than one tile of the accumulate kernel, a patch of more values than one staging holds
SWEEP = [((9, 11), 4, 1, np.float64), ((13, 17), (3, 5), 2, np.float64), ((21, 19), 4, 3, np.float64),
         ((8, 8), 8, 1, np.float64), ((7, 9), (7, 9), 4, np.float64), ((3, 10, 9), (4, 3), 3, np.float64),
         ((15, 14), 5, 2, np.float32), ((2, 9, 12), 2, 1, np.float32), ((70, 150), 4, 1, np.float64),
         ((41, 133), (8, 8), 5, np.float64), ((37, 45), 16, 1, np.float64), ((40, 200), (2, 40), 2, np.float64),
         ((5, 6), 1, 1, np.float64)]


def _image(rng, shape, dtype):
    return (rng.normal(size=shape) * 10.0 ** rng.randint(-2, 3, size=shape)).astype(dtype)


# --------------------------------------------------------------------------------------------------------- 3: extraction
@pytest.mark.parametrize("shape,patch,stride,dtype", SWEEP)
def test_extract_equals_the_reference_bit_for_bit(dev, shape, patch, stride, dtype):
    import torch
    from prosper_amd.utils import patches as U
    rng = np.random.RandomState(sum(shape) + stride)
    img = _image(rng, shape, dtype)
    want = P.extract(img, _pair(patch), stride)
    Y, means = U.extract_patches(img, patch, stride)
    assert means is None
    _same_bits(Y, want, "extract")
    # a row range that starts and ends mid-grid (inside patch rows), handed over as a range of the C entry
    geo = U._geometry(shape, patch, stride)
    N = len(want)
    t, ldi = U._image_tensor(img, dev)
    for n0, n in ((N // 3, N - N // 3 - N // 4), (N - 1, 1), (0, max(1, N // 2))):
        part, _ = U._extract(t, ldi, geo, n0, n, False, False)
        _same_bits(part.cpu().numpy(), want[n0:n0 + n], "rows [%d, %d)" % (n0, n0 + n))
    # an image held with a row stride (a view of a wider tensor) is read in place
    if len(shape) == 2:
        wide = torch.zeros((shape[0], shape[1] + 5), dtype=t.dtype, device=dev)
        wide[:, :shape[1]] = t[0]
        _same_bits(U.extract_patches(wide[:, :shape[1]], patch, stride)[0], want, "row stride")


@pytest.mark.parametrize("shape,patch,stride,dtype", SWEEP)
def test_extract_centred(dev, shape, patch, stride, dtype):
    """Y + means reproduces the uncentred rows to 1 ulp of the patch's largest value; the means agree with fsum / D within
    D 2^-53 max |patch| (D - 1 rounded additions in the header's fixed order, one division); a patch's bits do not depend
    on where in a chunk it sits."""
    from prosper_amd.utils import patches as U
    rng = np.random.RandomState(sum(shape) + stride + 1)
    img = _image(rng, shape, dtype)
    plain = P.extract(img, _pair(patch), stride)
    N, D = plain.shape
    Y, means = U.extract_patches(img, patch, stride, center=True)
    assert Y.shape == (N, D) and means.shape == (N,) and means.dtype == np.float64
    big = np.abs(plain).max(axis=1)
    exact = np.array([math.fsum(row) / D for row in plain])
    err_mean = np.abs(means - exact) / big
    err_back = np.abs(Y + means[:, None] - plain).max(axis=1) / big
    print("centred %s patch %s stride %d: mean error %.2f of D 2^-53 max|patch|, Y + mean error %.2f ulp" % (
        shape, patch, stride, err_mean.max() / (D * 2.0 ** -53), err_back.max() / 2.0 ** -52))
    assert (err_mean <= D * 2.0 ** -53).all()
    assert (err_back <= 2.0 ** -52).all()
    _same_bits(Y, plain - means[:, None], "x - mean, one rounding")
    geo = U._geometry(shape, patch, stride)
    t, ldi = U._image_tensor(img, dev)
    n0, n = N // 3, N - N // 3
    Yp, mp = U._extract(t, ldi, geo, n0, n, True, False)
    _same_bits(Yp.cpu().numpy(), Y[n0:], "centred rows of a range")
    _same_bits(mp.cpu().numpy(), means[n0:], "means of a range")


def test_the_same_patch_at_two_positions_gives_the_same_bits(dev):
    from prosper_amd.utils import patches as U
    rng = np.random.RandomState(4)
    one = _image(rng, (11, 13), np.float64)
    for patch in (3, (2, 5), 8):
        Y, means = U.extract_patches(np.stack([one, one, one]), patch, 2, center=True)
        N = len(Y) // 3
        for k in (1, 2):
            _same_bits(Y[k * N:(k + 1) * N], Y[:N])
            _same_bits(means[k * N:(k + 1) * N], means[:N])


# ------------------------------------------------------------------------------------------------------ 4: the average
@pytest.mark.parametrize("shape,patch,stride,dtype", SWEEP)
def test_average_equals_the_reference_bit_for_bit(dev, shape, patch, stride, dtype):
    import torch
    from prosper_amd.utils import patches as U
    rng = np.random.RandomState(sum(shape) + stride + 2)
    ph, pw = _pair(patch)
    N = len(P.grid(shape, (ph, pw), stride))
    E = rng.normal(size=(N, ph * pw)) * 10.0 ** rng.randint(-2, 3, size=(N, 1))
    mu = rng.normal(size=N) * 3
    _same_bits(U.average_patches(E, shape, patch, stride), P.average(E, shape, (ph, pw), stride), "average")
    _same_bits(U.average_patches(E, shape, patch, stride, means=mu), P.average(E, shape, (ph, pw), stride, means=mu),
               "average with means")
    # handed over in ranges that start and end inside patch rows, from an estimate matrix with a leading dimension
    geo = U._geometry(shape, patch, stride)
    full = geo[0]
    acc = torch.zeros(full, dtype=torch.float64, device=dev)
    wide = torch.full((N, ph * pw + 3), float("nan"), dtype=torch.float64, device=dev)
    wide[:, :ph * pw] = torch.from_numpy(E).to(dev)
    mu_d = torch.from_numpy(mu).to(dev)
    cuts = sorted(set([0, N // 5, N // 5 + 1, N // 2, N]))
    for a, b in zip(cuts, cuts[1:]):
        U._accumulate(acc, wide[a:], ph * pw + 3, mu_d[a:], geo, a, b - a, False)
    out = U._finish(acc, geo, False).cpu().numpy()
    _same_bits(out.reshape(shape), P.average(E, shape, (ph, pw), stride, means=mu), "average in ranges")


def test_both_builds_give_the_same_bits(dev):
    import torch
    from prosper_amd.utils import patches as U
    rng = np.random.RandomState(6)
    shape, patch, stride = (23, 31), (4, 6), 3
    img = torch.from_numpy(_image(rng, shape, np.float64)).to(dev)
    geo = U._geometry(shape, patch, stride)
    N = geo[3] * geo[4]
    outs = []
    for det in (False, True):
        Y, m = U._extract(img[None], shape[1], geo, 0, N, True, det)
        acc = torch.zeros((1,) + shape, dtype=torch.float64, device=dev)
        U._accumulate(acc, Y, 24, m, geo, 0, N, det)
        outs.append((Y.cpu().numpy(), m.cpu().numpy(), U._finish(acc, geo, det).cpu().numpy()))
    for a, b in zip(*outs):
        _same_bits(a, b)


# ---------------------------------------------------------------------------------------------- models on a small shape
EIGHT = ["bsc", "mca", "mmca", "dsc3", "tsc", "gsc_scalar", "mog_diagonal", "mop"]


def _model(name, D, H, Hp, g, seed=7):
    """(model, params) of tests/test_reconstruct_gpu.py's problems at D = p^2."""
    from test_reconstruct_gpu import _mixture, _problem
    rng = np.random.RandomState(seed)
    if name.startswith("mo"):
        m, p, _, _ = _mixture(name, rng, D, H, 4)
    else:
        m, p, _, _, _ = _problem(name, rng, D, H, 4, Hp, g)
    return m, p


# ---------------------------------------------------------------------------------------------------------- 5: composition
@pytest.mark.parametrize("name", EIGHT)
def test_denoise_image_is_extract_reconstruct_average(dev, name):
    from prosper_amd.utils import patches as U
    m, p = _model(name, 16, 6, 4, 3)
    rng = np.random.RandomState(3)
    img = rng.uniform(0.0, 3.0, size=(2, 14, 13))
    for stride, center in ((1, False), (3, False), (2, True)):
        Y, means = U.extract_patches(img, 4, stride, center=center)
        want = U.average_patches(m.reconstruct(p, {"y": Y}), img.shape, 4, stride, means=means)
        got = m.reconstruct_image(p, img, stride=stride, center=center)
        assert np.isfinite(got).all()
        _same_bits(got, want, "%s stride %d" % (name, stride))
        _same_bits(U.denoise_image(m, p, img, patch=(4, 4), stride=stride, center=center), want)
    _same_bits(m.reconstruct_image(p, img[0], patch=(2, 8), stride=2),
               U.average_patches(m.reconstruct(p, {"y": U.extract_patches(img[0], (2, 8), 2)[0]}), img[0].shape, (2, 8), 2))


# --------------------------------------------------------------------------------------------------- 6: chunk independence
@pytest.mark.parametrize("name", ["bsc", "mca", "gsc_scalar", "mog_diagonal"])
def test_the_result_does_not_depend_on_the_chunking(dev, name):
    m, p = _model(name, 16, 6, 4, 3)
    rng = np.random.RandomState(5)
    img = rng.uniform(0.0, 3.0, size=(2, 25, 22))
    for stride in (1, 3):
        nc = len(P.starts(22, 4, stride))
        whole = m.reconstruct_image(p, img, stride=stride)
        for chunk in (1, nc, 3 * nc + 1, 10 ** 9):     # one patch row (rounded up to it), one, an odd number, everything
            _same_bits(m.reconstruct_image(p, img, stride=stride, chunk=chunk), whole, "%s chunk %d" % (name, chunk))
        m.deterministic = True
        try:
            _same_bits(m.reconstruct_image(p, img, stride=stride, chunk=5 * nc), whole, "%s deterministic" % name)
        finally:
            m.deterministic = False


# ------------------------------------------------------------------- 7 + 8: against enumeration; denoising denoises
A_BAR, SIGMA, PI, PB = 3.0, 1.0, 0.2, 4


def _bars_problem(kind, seed):
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    from prosper_amd.em.camodels.mca_et import MCA_ET
    rng = np.random.RandomState(seed)
    clean, noisy, _, _ = P.bars_image(rng, 40, 37, A_BAR, PI, SIGMA, mca=kind == "mca")
    W = P.bars_W(PB, A_BAR)
    H = 2 * PB
    if kind == "mca":
        W = np.where(W < 0.05, 0.05, W)              # as check_params does
        return MCA_ET(PB * PB, H, H, H), {"W": W, "pi": PI, "sigma": SIGMA}, clean, noisy
    return BSC_ET(PB * PB, H, H, H), {"W": W, "pi": PI, "sigma": SIGMA}, clean, noisy


@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("kind", ["bsc", "mca"])
def test_against_enumeration_on_the_bars_image(dev, kind, stride):
    """H' = gamma = H = 2p at the generating parameters: the exact posterior mean of every patch, averaged."""
    m, p, clean, noisy = _bars_problem(kind, 0)
    Y = P.extract(noisy, (PB, PB), stride)
    if kind == "mca":
        rows = R.enum_mca(Y, p["W"], m._rho(1.0), False, PI, SIGMA)
    else:
        rows = R.enum_linear(Y, p["W"], SIGMA, [0., 1.], np.log([1 - PI, PI]))
    want = P.average(rows, noisy.shape, (PB, PB), stride)
    got = m.reconstruct_image(p, noisy, stride=stride)
    err = np.abs(got - want).max() / np.abs(want).max()
    print("reconstruct_image %s stride %d against enumeration: %.3e of max |image| (bound 1e-11)" % (kind, stride, err))
    assert got.shape == noisy.shape and got.dtype == np.float64
    assert err <= 1e-11, err


@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("kind,seed", [("bsc", s) for s in range(5)] + [("mca", s) for s in range(4)])
def test_denoising_denoises(dev, kind, seed, stride):
    """(a) MSE(denoised, clean) < MSE(noisy, clean); (b) MSE(denoised, clean) <= mean of average((Yhat - Y_clean)^2) (1 +
    1e-12): Jensen's inequality per pixel, which holds for any correct average."""
    from prosper_amd.utils import patches as U
    m, p, clean, noisy = _bars_problem(kind, seed)
    got = m.reconstruct_image(p, noisy, stride=stride)
    Yhat = m.reconstruct(p, {"y": U.extract_patches(noisy, PB, stride)[0]})
    Yc = P.extract(clean, (PB, PB), stride)
    per_patch = P.average((Yhat - Yc) ** 2, clean.shape, (PB, PB), stride).mean()
    mse_n, mse_d = float(((noisy - clean) ** 2).mean()), float(((got - clean) ** 2).mean())
    print("bars %s seed %d stride %d: MSE noisy %.4f -> denoised %.5f (per-patch bound %.5f, ratio %.2f)" % (
        kind, seed, stride, mse_n, mse_d, per_patch, mse_d / per_patch))
    assert mse_d < mse_n
    assert mse_d <= per_patch * (1 + 1e-12)


# -------------------------------------------------------------------------------------------- 9: the plumbing by itself
class _Identity(object):
    """reconstruct() hands its input back: denoise_image is then extract -> accumulate -> finish."""
    deterministic = False

    def __init__(self, D, device):
        self.D, self.device, self.calls = D, device, 0

    def reconstruct(self, model_params, my_data, device=False):
        from prosper_amd.em.camodels._device import DeviceArray
        assert device and isinstance(my_data["y"], DeviceArray) and my_data["y"].tensor.is_cuda
        self.calls += 1
        return my_data["y"]


@pytest.mark.parametrize("shape,patch,stride", [((40, 37), 4, 1), ((40, 37), 4, 3), ((2, 33, 70), (3, 5), 2), ((12, 12), 4, 1)])
def test_identity_model_gives_the_image_back(dev, shape, patch, stride):
    from prosper_amd.utils import patches as U
    ph, pw = _pair(patch)
    rng = np.random.RandomState(8)
    img = _image(rng, shape, np.float64)
    k = P.cover(shape, (ph, pw), stride).reshape(shape)
    stub = _Identity(ph * pw, dev)
    nc = len(P.starts(shape[-1], pw, stride))
    back = U.denoise_image(stub, {}, img, patch=patch, stride=stride, chunk=2 * nc)
    assert stub.calls > 1
    worst = (np.abs(back - img) / (k * 2.0 ** -52 * np.abs(img))).max()
    print("identity %s patch %s stride %d: worst |delta| = %.2f of k 2^-52 |pixel| (cover up to %d)" % (shape, patch, stride, worst, k.max()))
    assert (np.abs(back - img) <= k * 2.0 ** -52 * np.abs(img)).all()
    back = U.denoise_image(stub, {}, img, patch=patch, stride=stride, center=True, chunk=3 * nc)
    worst = (np.abs(back - img) / ((k + 2) * 2.0 ** -52 * np.abs(img).max())).max()
    print("identity centred: worst |delta| = %.3f of (k + 2) 2^-52 max |image|" % worst)
    assert (np.abs(back - img) <= (k + 2) * 2.0 ** -52 * np.abs(img).max()).all()


# ----------------------------------------------------------------------------------------------------------------- 10: NaN
@pytest.mark.parametrize("stride", [1, 3])
def test_a_nan_pixel_spoils_exactly_its_patches(dev, stride):
    m, p = _model("bsc", 16, 6, 4, 3)
    rng = np.random.RandomState(9)
    img = rng.uniform(0.0, 3.0, size=(20, 18))
    clean = m.reconstruct_image(p, img, stride=stride)
    for pix in ((7, 9), (0, 0), (19, 17), (13, 2)):
        bad = img.copy()
        bad[pix] = np.nan
        out = m.reconstruct_image(p, bad, stride=stride, chunk=40)
        mask = P.patches_containing(img.shape, (4, 4), stride, pix)
        assert mask[pix] and np.array_equal(np.isnan(out), mask), (pix, np.isnan(out).sum(), mask.sum())
        _same_bits(out[~mask], clean[~mask], "pixels outside the NaN pixel's patches")


# ------------------------------------------------------------------------------------------------ 11: training undisturbed
@pytest.mark.parametrize("name", ["bsc", "gsc_scalar", "mog_diagonal"])
def test_training_is_undisturbed_by_a_call_between_two_steps(dev, name):
    """Two EM steps on an image's own patches (the DeviceArray of extract_patches as my_data['y']) with a reconstruct_image
    call between them end in the same parameters, bit for bit, as without it."""
    from test_reconstruct_gpu import _schedule
    from prosper_amd.utils import patches as U
    rng = np.random.RandomState(10)
    _, noisy, _, _ = P.bars_image(rng, 48, 45, A_BAR, PI, SIGMA)
    other = rng.uniform(0.0, 3.0, size=(19, 23))
    Y, _ = U.extract_patches(noisy, PB, 1, device=True)
    assert Y.shape == (45 * 42, 16) and Y.tensor.is_cuda

    def run(interleave):
        m, p = _model(name, 16, 8, 5, 3, seed=11)
        m.deterministic = True
        if name == "bsc":
            assert m._fused()                                    # the one-kernel E-step is the path under test
        p = {k: np.array(v, copy=True) for k, v in p.items()}
        a = _schedule(2)
        for step in range(2):
            p = m.step(a, p, {"y": Y})
            if interleave and step == 0:
                hp = (getattr(m, "Hprime", None), getattr(m, "gamma", None))
                q = {k: np.array(v, copy=True) for k, v in p.items()}
                out = m.reconstruct_image(q, other, stride=2, chunk=30)
                assert out.shape == other.shape and np.isfinite(out).all()
                assert (getattr(m, "Hprime", None), getattr(m, "gamma", None)) == hp
                for k in q:
                    np.testing.assert_array_equal(q[k], p[k])
            a.next()
        return {k: np.array(v, copy=True) for k, v in p.items()}
    ref, got = run(False), run(True)
    for k in ref:
        np.testing.assert_array_equal(ref[k], got[k], err_msg=k)


# ------------------------------------------------------------------------------------------- 12: residency of in- and output
def test_device_inputs_and_outputs_stay_on_the_device(dev, monkeypatch):
    import torch
    from prosper_amd.em.camodels._device import DeviceArray
    from prosper_amd.utils import patches as U
    rng = np.random.RandomState(12)
    img = rng.uniform(0.0, 3.0, size=(17, 21))
    t = torch.from_numpy(img).to(dev)
    host = U.denoise_image(_Identity(16, dev), {}, img, chunk=20)
    Yh, mh = U.extract_patches(img, 4, 2, center=True)
    ah = U.average_patches(Yh, img.shape, 4, 2, means=mh)

    def no_host(self, *a, **k):
        raise AssertionError("a tensor was copied to the host")
    with monkeypatch.context() as mp:
        mp.setattr(torch.Tensor, "cpu", no_host)
        mp.setattr(torch.Tensor, "numpy", no_host)
        mp.setattr(torch.Tensor, "tolist", no_host)
        out = U.denoise_image(_Identity(16, dev), {}, t, chunk=20, device=True)
        out2 = U.denoise_image(_Identity(16, dev), {}, DeviceArray(t), chunk=20, device=True)
        Y, means = U.extract_patches(t, 4, 2, center=True, device=True)
        avg = U.average_patches(Y, img.shape, 4, 2, means=means, device=True)
    for o in (out, out2, Y, means, avg):
        assert isinstance(o, DeviceArray) and o.tensor.is_cuda and o.dtype == np.float64
    _same_bits(np.asarray(out), host)
    _same_bits(np.asarray(out2), host)
    _same_bits(np.asarray(Y), Yh)
    _same_bits(np.asarray(means), mh)
    _same_bits(np.asarray(avg), ah)
    # a model's reconstruct_image takes the device tensor too, and float32 images go to the kernel as they are
    m, p = _model("bsc", 16, 6, 4, 3)
    d = m.reconstruct_image(p, t, stride=2, device=True)
    assert isinstance(d, DeviceArray) and d.shape == img.shape
    _same_bits(np.asarray(d), m.reconstruct_image(p, img, stride=2))
    f32 = img.astype(np.float32)
    _same_bits(m.reconstruct_image(p, torch.from_numpy(f32).to(dev), stride=2), m.reconstruct_image(p, f32.astype(np.float64), stride=2))
    _same_bits(m.reconstruct_image(p, (img * 40).astype(np.int32), stride=2),
               m.reconstruct_image(p, (img * 40).astype(np.int32).astype(np.float64), stride=2))
