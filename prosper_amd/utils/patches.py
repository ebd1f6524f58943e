"""Whole-image denoising by overlapping patches: cut an image into p_h x p_w patches on the device, estimate
every patch with a model's ``reconstruct()``, put the estimates back and average where they overlap.  The patch matrix is
built, consumed and folded back on the device in chunks of whole patch rows (pm_patches_* of include/prosper_hip.h); there
is no CPU fallback.

The patch grid (one rule, used everywhere): along an axis of length L, patches of length p at stride s >= 1 start at 0, s,
2s, ... while start + p <= L, plus at L - p if the last of these is not L - p: every pixel is covered for every stride
s <= p (a larger stride would leave gaps between the regular starts and is refused where an image is cut).  Patches are
numbered row-major over (image, start row, start column); inside a patch the D = p_h p_w values are row-major, (a, b) ->
a p_w + b.

Feature maps: ``encode_image`` runs every patch through a model's ``encode()`` instead and returns the codes as
H channels on the patch grid, or pooled over a coarse grid of regions (``pool_regions``, ``pool_codes``; pm_codes_pool_*)."""
import ctypes

import numpy as np

from .. import _lib

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

CHUNK_BYTES = 1 << 30      # default budget of one chunk of denoise_image: its input rows plus its output rows
# aggregate='precision' weighs a patch's estimate of a pixel by 1 / (V + floor); floor=None: this times the model's noise
# variance.  Chosen on the MI355X from {1, 0.3, 0.1, 0.03, 0.01} by the table of DESIGN 4.21: the largest mean gain in PSNR
# over the mean aggregate on the four example runs (it is the grid's smallest value; the gain was still growing there).
PRECISION_FLOOR = 0.01
AGGREGATES = ("mean", "precision")


def patch_starts(length, patch, stride=1):
    """The patch starts along an axis of ``length`` positions, as a list (the grid rule of the module docstring)."""
    length, patch, stride = int(length), int(patch), int(stride)
    if patch < 1 or stride < 1:
        raise ValueError("patch and stride must be at least 1 (got patch=%d, stride=%d)" % (patch, stride))
    if length < patch:
        raise ValueError("an axis of length %d holds no patch of length %d" % (length, patch))
    starts = list(range(0, length - patch + 1, stride))
    if starts[-1] != length - patch:
        starts.append(length - patch)
    return starts


def _patch_pair(patch):
    if isinstance(patch, (tuple, list, np.ndarray)):
        if len(patch) != 2:
            raise ValueError("patch is an int or a pair (p_h, p_w), got %r" % (patch,))
        ph, pw = int(patch[0]), int(patch[1])
    else:
        ph = pw = int(patch)
    if ph < 1 or pw < 1:
        raise ValueError("patch sides must be at least 1, got %r" % (patch,))
    return ph, pw


def _geometry(shape, patch, stride):
    """((B, Hi, Wi), (ph, pw), stride, nr, nc) of an image shape, or ValueError."""
    shape = tuple(int(v) for v in shape)
    if len(shape) == 2:
        shape = (1,) + shape
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError("an image is (H, W) or a stack (B, H, W) with no empty axis, got shape %r (colour channels are "
                         "out of scope)" % (shape,))
    ph, pw = _patch_pair(patch)
    if int(stride) != stride or int(stride) < 1:
        raise ValueError("stride must be an integer >= 1, got %r" % (stride,))
    nr, nc = len(patch_starts(shape[1], ph, stride)), len(patch_starts(shape[2], pw, stride))
    for L, p in ((shape[1], ph), (shape[2], pw)):
        if stride > p and L > 2 * p:
            raise ValueError("stride %d leaves pixels between patches of length %d uncovered on an axis of length %d: an "
                             "average needs stride <= patch" % (stride, p, L))
    return shape, (ph, pw), int(stride), nr, nc


def _shape_of(a):
    t = getattr(a, "tensor", a)
    return tuple(t.shape)


def _device(model=None):
    if getattr(model, "device", None) is not None:
        return torch.device(model.device)
    if torch is None or not torch.cuda.is_available():
        raise _lib.HipError("the patch kernels need a HIP device: there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _image_tensor(image, dev):
    """The (B, Hi, Wi) float32 / float64 device tensor of ``image`` with unit column stride and images Hi rows apart, and its
    row stride.  A device tensor that already has this layout is used in place."""
    t = getattr(image, "tensor", image)
    if torch.is_tensor(t):
        if t.dtype not in (torch.float32, torch.float64):
            t = t.cpu().to(torch.float64)
    else:
        t = np.asarray(t)
        if t.dtype not in (np.float32, np.float64):
            t = t.astype(np.float64)
        t = torch.from_numpy(np.ascontiguousarray(t))
    t = t.to(dev)
    if t.dim() == 2:
        t = t.unsqueeze(0)
    B, Hi, Wi = t.shape
    if t.stride(2) != 1 or t.stride(1) < Wi or (B > 1 and t.stride(0) != Hi * t.stride(1)):
        t = t.contiguous()
    return t, int(t.stride(1)) if Hi > 1 else max(int(t.stride(1)), Wi)


def _rows_tensor(Y, D, dev, what):
    """An (n, D) float64 device tensor with unit column stride of ``Y`` (host array, tensor or DeviceArray), and its leading
    dimension."""
    t = getattr(Y, "tensor", Y)
    if not torch.is_tensor(t):
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(t), dtype=np.float64))
    if t.dim() != 2 or t.shape[1] != D:
        raise ValueError("%s must be (N, %d), got %r" % (what, D, tuple(t.shape)))
    t = t.to(device=dev, dtype=torch.float64)
    if t.stride(1) != 1 or t.stride(0) < D:
        t = t.contiguous()
    return t, int(t.stride(0)) if t.shape[0] > 1 else max(int(t.stride(0)), D)


def _extract(img, ldi, geo, n0, n, center, det):
    (B, Hi, Wi), (ph, pw), stride, nr, nc = geo
    dev = img.device
    Y = torch.empty((n, ph * pw), dtype=torch.float64, device=dev)
    means = torch.empty(n, dtype=torch.float64, device=dev) if center else None
    entry = "pm_patches_extract_f32" if img.dtype == torch.float32 else "pm_patches_extract_f64"
    _lib.call(entry, _ptr(img), ldi, B, Hi, Wi, ph, pw, stride, n0, n, int(bool(center)), _ptr(Y), ph * pw, _ptr(means),
              _stream(dev), det=det)
    return Y, means


def _accumulate(acc, est, lde, means, geo, n0, n, det):
    (B, Hi, Wi), (ph, pw), stride, nr, nc = geo
    _lib.call("pm_patches_accumulate_f64", _ptr(est), lde, _ptr(means), n0, n, _ptr(acc), Wi, B, Hi, Wi, ph, pw, stride,
              _stream(acc.device), det=det)


def _finish(acc, geo, det):
    (B, Hi, Wi), (ph, pw), stride, nr, nc = geo
    out = torch.empty_like(acc)
    _lib.call("pm_patches_finish_f64", _ptr(acc), Wi, _ptr(out), Wi, B, Hi, Wi, ph, pw, stride, _stream(acc.device), det=det)
    return out


def _accumulate_w(num, den, est, lde, wgt, ldw, wmode, floor, window, means, geo, n0, n, det):
    """pm_patches_accumulate_w_f64: num += w est (+ means), den += w (den None: skipped); w from ``wgt`` (None, or
    (n, ldw) used as given -- wmode 0 -- or as variances, 1 / (max(V, 0) + floor) -- wmode 1) times ``window`` (None or (D,))."""
    (B, Hi, Wi), (ph, pw), stride, nr, nc = geo
    _lib.call("pm_patches_accumulate_w_f64", _ptr(est), lde, _ptr(wgt), ldw, wmode, float(floor), _ptr(window), _ptr(means),
              n0, n, _ptr(num), _ptr(den), Wi, B, Hi, Wi, ph, pw, stride, _stream(num.device), det=det)


def _finish_w(num, den, geo, det):
    (B, Hi, Wi) = geo[0]
    out = torch.empty_like(num)
    _lib.call("pm_patches_finish_w_f64", _ptr(num), _ptr(den), Wi, _ptr(out), Wi, B, Hi, Wi, _stream(num.device), det=det)
    return out


def _window_host(window, ph, pw):
    """The (D,) float64 host array of ``window`` ((p_h, p_w) or (D,); every entry finite and > 0), or ValueError."""
    w = getattr(window, "tensor", window)
    if torch is not None and torch.is_tensor(w):
        w = w.detach().cpu().numpy()
    w = np.asarray(w, dtype=np.float64)
    if w.shape not in ((ph, pw), (ph * pw,)):
        raise ValueError("window must be (%d, %d) or (%d,), got %r" % (ph, pw, ph * pw, w.shape))
    if not (np.isfinite(w).all() and (w > 0).all()):
        raise ValueError("every entry of window must be finite and > 0")
    return np.ascontiguousarray(w.reshape(-1))


def _hand_back(t, squeeze, device):
    from ..em.camodels._device import DeviceArray
    if t is None:
        return None
    if squeeze:
        t = t[0]
    return DeviceArray(t) if device else t.cpu().numpy()


def extract_patches(image, patch, stride=1, center=False, device=False):
    """The (N, D) float64 patch matrix of ``image`` -- (H_i, W_i) or a stack (B, H_i, W_i); NumPy array, torch tensor (a
    device tensor is read in place) or ``DeviceArray``; float32 and float64 go to the kernel as they are, other types are
    converted to float64 on the host -- on the grid of the module docstring, built on the device by pm_patches_extract_*.

    Returns ``(Y, means)``: ``means`` is None, or with ``center=True`` the (N,) patch means, ``Y`` then holding each patch
    minus its mean.  NumPy arrays, or with ``device=True`` ``DeviceArray``s left on the device: ``Y`` is accepted as
    ``my_data['y']`` by ``EM``, ``model.step``, ``reconstruct`` and ``log_likelihood`` as it is."""
    geo = _geometry(_shape_of(image), patch, stride)
    dev = _device()
    img, ldi = _image_tensor(image, dev)
    Y, means = _extract(img, ldi, geo, 0, geo[0][0] * geo[3] * geo[4], center, False)
    return _hand_back(Y, False, device), _hand_back(means, False, device)


def average_patches(Y, image_shape, patch, stride=1, means=None, device=False, weights=None, window=None):
    """Put the (N, D) patches ``Y`` (+ their ``means`` (N,), if given) back onto an image of ``image_shape`` ((H_i, W_i) or
    (B, H_i, W_i)) and average where they overlap: every pixel is the sum of its patches' values, added one at a time in
    ascending patch number, divided by their number (pm_patches_accumulate_f64, pm_patches_finish_f64; no atomics, the same
    bits on every run).  Returns the float64 image as a NumPy array, or with ``device=True`` as a ``DeviceArray``.

    ``weights`` ((N, D); NumPy, torch or ``DeviceArray``; used as given) and / or ``window`` ((p_h, p_w) or (D,), every entry
    finite and > 0, else ``ValueError``) make it the weighted average of DESIGN 4.21: element e of patch k weighs w =
    weights[k, e] window[e] (a factor that is not given is not multiplied), every pixel is sum (w value) / sum w, both sums
    added in ascending patch number, each product rounded before it is added (pm_patches_accumulate_w_f64,
    pm_patches_finish_w_f64).  A pixel all of whose weights are 0 is NaN.  With neither keyword the call is the plain one."""
    geo = _geometry(image_shape, patch, stride)
    (B, Hi, Wi), (ph, pw), _, nr, nc = geo
    N = B * nr * nc
    if _shape_of(Y) != (N, ph * pw):
        raise ValueError("Y must be (%d, %d) for this image, patch and stride, got %r" % (N, ph * pw, _shape_of(Y)))
    if means is not None and _shape_of(means) != (N,):
        raise ValueError("means must be (%d,), got %r" % (N, _shape_of(means)))
    if weights is not None and _shape_of(weights) != (N, ph * pw):
        raise ValueError("weights must be (%d, %d), got %r" % (N, ph * pw, _shape_of(weights)))
    win = _window_host(window, ph, pw) if window is not None else None
    dev = _device()
    est, lde = _rows_tensor(Y, ph * pw, dev, "Y")
    if means is not None:
        means = getattr(means, "tensor", means)
        if not torch.is_tensor(means):
            means = torch.from_numpy(np.ascontiguousarray(np.asarray(means), dtype=np.float64))
        means = means.to(device=dev, dtype=torch.float64).contiguous()
    acc = torch.zeros((B, Hi, Wi), dtype=torch.float64, device=dev)
    if weights is not None or win is not None:
        wgt, ldw = _rows_tensor(weights, ph * pw, dev, "weights") if weights is not None else (None, 0)
        win = torch.from_numpy(win).to(dev) if win is not None else None
        den = torch.zeros_like(acc)
        _accumulate_w(acc, den, est, lde, wgt, ldw, 0, 0.0, win, means, geo, 0, N, False)
        return _hand_back(_finish_w(acc, den, geo, False), len(tuple(image_shape)) == 2, device)
    _accumulate(acc, est, lde, means, geo, 0, N, False)
    return _hand_back(_finish(acc, geo, False), len(tuple(image_shape)) == 2, device)


def _mask_image(mask, shape, dev):
    """The 0 / 1 float64 device image of ``mask`` (non-zero = observed; any type ``_image_tensor`` reads), cut into patches
    by the extraction kernel like the image itself."""
    if _shape_of(mask) != tuple(shape):
        raise ValueError("mask has shape %r, the image %r" % (_shape_of(mask), tuple(shape)))
    t = getattr(mask, "tensor", mask)
    if not torch.is_tensor(t):
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(t) != 0))
    return _image_tensor((t.to(dev) != 0).to(torch.float64), dev)


def _weight_check(weight):
    """``ValueError`` naming the weight unless every entry is finite and >= 0: one reduction where the weight lives (NaN fails
    the first comparison)."""
    t = getattr(weight, "tensor", weight)
    if torch is not None and torch.is_tensor(t):
        v = t.to(torch.uint8) if t.dtype == torch.bool else t
        ok = bool(((v >= 0) & (v < float("inf"))).all())
    else:
        with np.errstate(invalid="ignore"):
            t = np.asarray(t)
            ok = bool(np.all((t >= 0) & (t < np.inf)))
    if not ok:
        raise ValueError("every entry of 'weight' must be finite and >= 0 (0 = not observed): a weight is never clamped")


def _weight_image(weight, dev):
    """The float64 device image of ``weight`` (any type ``_image_tensor`` reads), cut into patches by the extraction kernel
    like the image itself."""
    t = getattr(weight, "tensor", weight)
    if not torch.is_tensor(t):
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(t), dtype=np.float64))
    return _image_tensor(t.to(device=dev, dtype=torch.float64), dev)


def denoise_image(model, model_params, image, patch=None, stride=1, center=False, chunk=None, device=False, mask=None,
                  exact=False, variance=False, aggregate='mean', floor=None, window=None, weight=None):
    """Denoise ``image`` ((H_i, W_i) or a stack (B, H_i, W_i); NumPy array, torch tensor -- a device tensor is used in place,
    without a host round trip -- or ``DeviceArray``) with ``model`` at ``model_params``: every overlapping patch on the grid of
    the module docstring is replaced by its posterior mean ``model.reconstruct()`` and every pixel by the average of the
    estimates of the patches that contain it, added in ascending patch number.

    ``patch``: an int or a pair (p_h, p_w) with p_h p_w = model.D; None: the square patch with p^2 = model.D.  ``center``:
    each patch's mean is removed before the model sees it and added back to its estimate.  The patches are walked in chunks
    of whole patch rows: extract -> ``model.reconstruct(model_params, {'y': chunk}, device=True)`` -> accumulate, then one
    division per pixel.  ``chunk``: patches per chunk, rounded down to whole patch rows (at least one); None: as many patch
    rows as keep a chunk's input rows plus output rows within 1 GiB (``CHUNK_BYTES``).  Device memory is bounded by the chunk,
    not by the image, and the result's bits do not depend on ``chunk`` (a row of ``reconstruct()`` depends on that row and the
    parameters alone; the additions of a pixel run in the same order for every chunking).

    It inherits from ``reconstruct()``: this rank's images only, no collective; the training state, ``model_params`` and
    Hprime / gamma are left as they were; MoP with ``A`` set works in the normalised units ``reconstruct()`` documents; every
    ``HipError`` limit of ``reconstruct()`` applies.  A NaN pixel makes NaN exactly the pixels of the patches that contain it.

    ``mask`` (missing values): an array of the image's shape, non-zero = observed pixel.  Its patches are cut on
    the same grid and every chunk goes through ``model.reconstruct(model_params, {'y': chunk, 'mask': chunk's mask})``: the
    unobserved pixels of a patch leave its likelihood and are read from its estimate (inpainting), whatever the image holds
    there -- NaN included.  The overlap average is unchanged and covers every pixel.  ``center=True`` with a mask raises
    ``ValueError`` (a mean over the observed pixels only is not built); a model without the masked E-step raises
    ``NotImplementedError``.

    ``weight`` (per-pixel noise weights): an array of the image's shape, finite and >= 0: pixel (i, j) was observed
    with noise variance sigma^2 / weight[i, j], 0 = not observed.  Its patches are cut on the same grid by the same kernel, kept
    as float64, and every chunk goes through ``model.reconstruct(model_params, {'y': chunk, 'weight': chunk's weights})``;
    ``aggregate``, ``variance``, ``window``, stacks and ``chunk`` work as without it and the bits do not depend on ``chunk``.
    What the image holds at weight 0 changes no bit.  A weight that is negative, NaN or infinite anywhere, one of another
    shape, ``weight`` together with ``mask`` (fold the mask into the weight as zeros) and ``center=True`` raise
    ``ValueError``, ``exact=True`` and a model without the weighted E-step ``NotImplementedError`` -- all before any launch.

    ``exact=True``: every patch through ``model.reconstruct(..., exact=True)``, the posterior mean over the
    model's whole state space; its limits apply, and with a mask it raises ``NotImplementedError``.  The keyword reaches
    ``reconstruct()`` only when it is set.

    ``variance=True``: every patch through ``model.reconstruct(..., variance=True)`` and the result is ``(image,
    var_map)``; the image has the bits of the call without the keyword.  ``var_map`` is the overlap average of the patches'
    posterior variances V through the same accumulate / finish kernels (the same bits for every ``chunk``): the MEAN OF THE
    COVERING PATCHES' VARIANCES.  Whatever the correlation between the patches' estimates, Var(mean) <= mean Var, so it is an
    upper bound on the variance of the averaged estimate, not that variance itself.  It is the variance of the noiseless
    value; ``center=True`` leaves V unchanged (the patch mean is a constant to the model).  The keyword reaches
    ``reconstruct()`` only when it is set.

    ``aggregate``: how the overlapping estimates of a pixel are combined.  ``'mean'`` (default): equal weights,
    the calls and the bits above.  ``'precision'``: every chunk goes through ``model.reconstruct(..., variance=True)`` and a
    patch's estimate of a pixel weighs w = 1 / (max(V, 0) + floor), V its posterior variance there: pixel = sum (w estimate) /
    sum w over the covering patches in ascending patch number (pm_patches_accumulate_w_f64, pm_patches_finish_w_f64), so a
    pixel that one patch does not observe and a neighbouring patch constrains well follows the confident one.  ``floor``: a
    finite number > 0 (else ``ValueError``) that keeps a weight finite at V = 0 and sets how far the weights may spread -- at
    floor >> V they are uniform, towards 0 the most confident patch takes all; None: ``PRECISION_FLOOR`` times
    ``model._noise_variance(model_params)`` (sigma^2; the mean diagonal for GSC and MoG; MoP has no noise parameter and raises
    ``ValueError`` asking for ``floor=``).  ``window`` ((p_h, p_w) or (D,), finite and > 0, else ``ValueError``): a fixed
    weight per patch element that multiplies w, or is the weight under ``'mean'`` (a window that falls off towards the
    patch's border trusts a patch most at its centre).  ``center``, ``mask``, stacks and ``chunk`` work as above
    (``center=True`` adds the patch mean to the estimate, V is unchanged), and the bits do not depend on ``chunk``.  With
    ``variance=True`` a weighted aggregate returns ``var_map = sum (w V) / sum w`` with the same weights: for fixed convex
    weights Var(sum w_k x_k) <= sum w_k Var(x_k) whatever the correlation between the estimates (Jensen's inequality), so it
    is still an upper bound on the variance of the aggregate, the weights taken as fixed -- a bound under the model's
    posterior, not on the error: it weighs the patches with the smallest V most and reads below the mean aggregate's map.
    ``aggregate='precision'`` with ``exact=True`` raises ``NotImplementedError``; any other ``aggregate`` string raises
    ``ValueError``.
    Returns the float64 image (the shape of ``image``) as a NumPy array, or with ``device=True`` as a ``DeviceArray``."""
    from ..em.camodels._device import DeviceArray
    if mask is not None and center:
        raise ValueError("center=True with a mask is not built: the patch mean would have to run over the observed pixels only")
    if weight is not None and mask is not None:
        raise ValueError("'weight' together with 'mask': fold the mask into the weight as zeros (weight = 0 where mask == 0)")
    if weight is not None and center:
        raise ValueError("center=True with a weight is not built: the patch mean would have to be the weighted one")
    D = int(model.D)
    if patch is None:
        p = int(round(D ** 0.5))
        if p * p != D:
            raise ValueError("model.D = %d is not a square: give patch=(p_h, p_w)" % D)
        patch = (p, p)
    ph, pw = _patch_pair(patch)
    if ph * pw != D:
        raise ValueError("a %d x %d patch has %d values, model.D is %d" % (ph, pw, ph * pw, D))
    shape = _shape_of(image)
    geo = _geometry(shape, (ph, pw), stride)
    (B, Hi, Wi), _, _, nr, nc = geo
    if chunk is None:
        chunk = CHUNK_BYTES // (16 * D)
    elif int(chunk) != chunk or int(chunk) < 1:
        raise ValueError("chunk must be a positive number of patches, got %r" % (chunk,))
    rows = max(1, int(chunk) // nc)
    extra = {'exact': True} if exact else {}
    if variance:
        extra['variance'] = True
    if mask is not None:
        if _shape_of(mask) != tuple(shape):
            raise ValueError("mask has shape %r, the image %r" % (_shape_of(mask), tuple(shape)))
        # (an empty masked call: a model without the masked E-step refuses here, before anything reaches the device)
        model.reconstruct(model_params, {'y': np.empty((0, D)), 'mask': np.empty((0, D), dtype=bool)}, **extra)
    if weight is not None:
        if _shape_of(weight) != tuple(shape):
            raise ValueError("weight has shape %r, the image %r" % (_shape_of(weight), tuple(shape)))
        _weight_check(weight)
        # (an empty weighted call: a model without the weighted E-step refuses here, before anything reaches the device)
        model.reconstruct(model_params, {'y': np.empty((0, D)), 'weight': np.empty((0, D))}, **extra)
    if variance and exact:
        raise NotImplementedError("denoise_image: variance=True with exact=True is not built (the enumeration kernels keep no "
                                  "second moments)")
    if aggregate not in AGGREGATES:
        raise ValueError("aggregate is 'mean' or 'precision', got %r" % (aggregate,))
    win = _window_host(window, ph, pw) if window is not None else None
    if floor is not None:
        try:
            floor = float(floor)
        except (TypeError, ValueError):
            raise ValueError("floor must be a finite number > 0, got %r" % (floor,))
        if not (np.isfinite(floor) and floor > 0.0):
            raise ValueError("floor must be a finite number > 0, got %r" % (floor,))
    precision = aggregate == 'precision'
    if precision and exact:
        raise NotImplementedError("denoise_image: aggregate='precision' with exact=True is not built (it needs the posterior "
                                  "variance, which the enumeration kernels do not return)")
    if precision and floor is None:
        floor = PRECISION_FLOOR * float(model._noise_variance(model_params))
        if not (np.isfinite(floor) and floor > 0.0):
            raise ValueError("the model's noise variance gives the floor %r: give floor= (a finite number > 0)" % (floor,))
    weighted = precision or win is not None
    if precision:
        extra['variance'] = True
    dev = _device(model)
    det = bool(getattr(model, "deterministic", False))
    img, ldi = _image_tensor(image, dev)
    mimg, ldmi = _mask_image(mask, shape, dev) if mask is not None else (None, 0)
    wimg, ldwi = _weight_image(weight, dev) if weight is not None else (None, 0)
    acc = torch.zeros((B, Hi, Wi), dtype=torch.float64, device=dev)
    vacc = torch.zeros((B, Hi, Wi), dtype=torch.float64, device=dev) if variance else None
    den = torch.zeros((B, Hi, Wi), dtype=torch.float64, device=dev) if weighted else None
    win = torch.from_numpy(win).to(dev) if win is not None else None
    for R0 in range(0, B * nr, rows):
        n0, n = R0 * nc, min(rows, B * nr - R0) * nc
        Y, means = _extract(img, ldi, geo, n0, n, center, det)
        data = {'y': DeviceArray(Y)}
        if mimg is not None:
            data['mask'] = DeviceArray((_extract(mimg, ldmi, geo, n0, n, False, det)[0] != 0).view(torch.uint8))
        if wimg is not None:
            data['weight'] = DeviceArray(_extract(wimg, ldwi, geo, n0, n, False, det)[0])
        est = model.reconstruct(model_params, data, device=True, **extra)
        del Y, data
        var, ldv = None, 0
        if variance or precision:
            est, var = est
            if _shape_of(var) != (n, D):
                raise ValueError("reconstruct() returned a variance of %r for a chunk of (%d, %d)" % (_shape_of(var), n, D))
            var, ldv = _rows_tensor(var, D, dev, "reconstruct()'s variance")
        if _shape_of(est) != (n, D):
            raise ValueError("reconstruct() returned %r for a chunk of (%d, %d)" % (_shape_of(est), n, D))
        est, lde = _rows_tensor(est, D, dev, "reconstruct()'s result")
        if weighted:
            # the weights: 1 / (max(V, 0) + floor) under 'precision', times the window; under 'mean' the window alone
            wgt, ldw, wmode, fl = (var, ldv, 1, floor) if precision else (None, 0, 0, 0.0)
            if variance:
                _accumulate_w(vacc, None, var, ldv, wgt, ldw, wmode, fl, win, None, geo, n0, n, det)
            _accumulate_w(acc, den, est, lde, wgt, ldw, wmode, fl, win, means, geo, n0, n, det)
        else:
            if variance:
                _accumulate(vacc, var, ldv, None, geo, n0, n, det)
            _accumulate(acc, est, lde, means, geo, n0, n, det)
        del est, means, var
    if weighted:
        out = _hand_back(_finish_w(acc, den, geo, det), len(shape) == 2, device)
        if variance:
            return out, _hand_back(_finish_w(vacc, den, geo, det), len(shape) == 2, device)
        return out
    out = _hand_back(_finish(acc, geo, det), len(shape) == 2, device)
    if variance:
        return out, _hand_back(_finish(vacc, geo, det), len(shape) == 2, device)
    return out


# ---- pooled feature maps of an image's patch codes ------------------------------------------------------------
REDUCES = ("mean", "sum", "max")


def pool_regions(n, g):
    """The ``g`` regions of an axis of ``n`` patch positions, as a list of ``(start, stop)``: region i is [floor(i n / g),
    floor((i + 1) n / g)) -- ascending, never empty, lengths differing by at most 1.  ``ValueError`` unless 1 <= g <= n.  The
    one region rule: pm_codes_pool_f64 (include/prosper_hip.h) and the tests' reference cut the same way."""
    if int(n) != n or int(g) != g or not 1 <= int(g) <= int(n):
        raise ValueError("an axis of %r patch positions is cut into 1 <= g <= n regions, got g = %r" % (n, g))
    n, g = int(n), int(g)
    return [(i * n // g, (i + 1) * n // g) for i in range(g)]


def _pool_pair(pool, nr, nc):
    """(gh, gw) of ``pool`` (an int g meaning (g, g), or a pair) on an (nr, nc) patch grid, or ValueError."""
    if isinstance(pool, (tuple, list, np.ndarray)):
        if len(pool) != 2:
            raise ValueError("pool is an int or a pair (gh, gw), got %r" % (pool,))
        gh, gw = pool
    else:
        gh = gw = pool
    try:
        ok = int(gh) == gh and int(gw) == gw
    except (TypeError, ValueError):
        ok = False
    if not ok or int(gh) < 1 or int(gw) < 1:
        raise ValueError("pool is an int or a pair (gh, gw) of integers >= 1, got %r" % (pool,))
    if int(gh) > nr or int(gw) > nc:
        raise ValueError("pool=(%d, %d) has more regions than the (%d, %d) patch grid has positions" % (gh, gw, nr, nc))
    return int(gh), int(gw)


def _reduce_check(reduce):
    if not isinstance(reduce, str) or reduce not in REDUCES:
        raise ValueError("reduce is 'mean', 'sum' or 'max', got %r" % (reduce,))


def _pool_begin(grid, pool, H, reduce, dev):
    """The running result (B, gh, gw, H) of pm_codes_pool_f64: +0 for a sum, -inf for a maximum."""
    return torch.full((grid[0], pool[0], pool[1], H), float("-inf") if reduce == 'max' else 0.0, dtype=torch.float64,
                      device=dev)


def _pool_work(rows, nc, gw, H, dev):
    """The scratch of pm_codes_pool_f64 for ranges of at most ``rows`` patch rows."""
    return torch.empty(max(int(_lib.load().pm_codes_pool_work_len(rows * nc, nc, gw, H)), 1), dtype=torch.float64, device=dev)


def _pool(acc, codes, ldc, grid, pool, n0, n, reduce, work, det):
    (B, nr, nc), (gh, gw) = grid, pool
    _lib.call("pm_codes_pool_f64", _ptr(codes), ldc, n0, n, B, nr, nc, gh, gw, acc.shape[3], int(reduce == 'max'), _ptr(acc),
              _ptr(work), _stream(acc.device), det=det)


def _pool_finish(acc, grid, pool, reduce, det):
    """The mean's one division per output, in place; a sum or a maximum is the running result itself."""
    if reduce == 'mean':
        (B, nr, nc), (gh, gw) = grid, pool
        _lib.call("pm_codes_pool_finish_f64", _ptr(acc), _ptr(acc), B, nr, nc, gh, gw, acc.shape[3], _stream(acc.device),
                  det=det)
    return acc


def pool_codes(codes, grid, pool, reduce='mean', device=False):
    """Pool the (N, H) ``codes`` (NumPy, torch or ``DeviceArray``) of the patches of a grid ``(B, nr, nc)``, N = B nr nc,
    numbered as the module docstring says, over ``pool = (gh, gw)`` regions (an int g: (g, g)): the (B, gh, gw, H) float64
    array whose entry (b, i, j, h) reduces channel h over the patches of image b with start-row index in
    ``pool_regions(nr, gh)[i]`` and start-column index in ``pool_regions(nc, gw)[j]``.  The aggregation of ``encode_image`` on
    its own, as ``average_patches`` is that of ``denoise_image``.

    ``reduce``: ``'sum'`` -- per patch row the region's columns are added one at a time in ascending order starting from +0,
    and the patch rows' sums are added one at a time in ascending order (pm_codes_pool_f64: no atomics, the same bits on
    every run and for every split into chunks); ``'mean'`` -- that sum divided once by the number of patches of the region;
    ``'max'`` -- the largest value, a NaN input making that output NaN (and max(-0, +0) = +0).  Anything else, a grid or
    ``pool`` that does not fit and codes of another shape raise ``ValueError`` before any device call.  Returns a NumPy array,
    or with ``device=True`` a ``DeviceArray``."""
    _reduce_check(reduce)
    try:
        B, nr, nc = (int(v) for v in grid)
    except (TypeError, ValueError):
        raise ValueError("grid is (B, nr, nc), got %r" % (grid,))
    if min(B, nr, nc) < 1:
        raise ValueError("grid is (B, nr, nc) with no empty axis, got %r" % (grid,))
    pool = _pool_pair(pool, nr, nc)
    shape = _shape_of(codes)
    if len(shape) != 2 or shape[0] != B * nr * nc or shape[1] < 1:
        raise ValueError("codes must be (%d, H >= 1) for the grid %r, got %r" % (B * nr * nc, (B, nr, nc), shape))
    H = int(shape[1])
    dev = _device()
    t, ldc = _rows_tensor(codes, H, dev, "codes")
    acc = _pool_begin((B, nr, nc), pool, H, reduce, dev)
    _pool(acc, t, ldc, (B, nr, nc), pool, 0, B * nr * nc, reduce, _pool_work(B * nr, nc, pool[1], H, dev), False)
    return _hand_back(_pool_finish(acc, (B, nr, nc), pool, reduce, False), False, device)


def encode_image(model, model_params, image, patch=None, stride=1, center=False, chunk=None, device=False, mask=None,
                 weight=None, exact=False, pool=None, reduce='mean'):
    """The feature maps of ``image`` ((H_i, W_i) or a stack (B, H_i, W_i); NumPy array, torch tensor -- a device tensor is
    used in place -- or ``DeviceArray``) under ``model`` at ``model_params``: every patch on the grid of the module docstring
    through ``model.encode()``.  Returns ``(mean, prob)``, the two codes ``encode()`` documents, as H channels on the patch
    grid, channel-last: (B, nr, nc, H) float64 for a stack, (nr, nc, H) for a 2-D image -- ``encode()`` of the whole patch
    matrix, reshaped, bit for bit.  Codes are not overlap-averaged: a patch keeps its own.

    ``image``, ``patch``, ``stride``, ``center``, ``mask``, ``weight`` and ``device`` mean what they mean in
    ``denoise_image``: the same grid (stride <= patch), ``center`` removes each patch's mean before the model sees it, a
    ``mask`` / ``weight`` of the image's shape is cut into patches by the same kernel and every chunk goes through
    ``model.encode(model_params, {'y': chunk, 'mask' | 'weight': ...})`` (BSC, MCA, MMCA; what the image holds under a hole or
    at weight 0 changes no bit).  ``center=True`` with a mask or a weight, ``weight`` together with ``mask`` and a weight that
    is negative, NaN or infinite raise ``ValueError``, a model without the masked / weighted E-step ``NotImplementedError`` --
    all before any launch.  ``exact=True`` reaches ``encode()`` only when it is set; ``encode()``'s own refusals and
    ``HipError`` limits apply unchanged.

    The patches are walked in chunks of whole patch rows: extract -> ``model.encode(..., device=True)`` -> write into the
    preallocated maps, or pool.  ``chunk``: patches per chunk, rounded down to whole patch rows (at least one); None: as many
    patch rows as keep a chunk's input rows plus its two code rows, 8 (D + 2 H) bytes per patch, within ``CHUNK_BYTES``.
    The result's bits do not depend on ``chunk``.

    ``pool=(gh, gw)`` (an int g: (g, g); ``ValueError`` if gh > nr or gw > nc): both results are pooled over a gh x gw grid of
    regions into (B, gh, gw, H) -- (gh, gw, H) for a 2-D image --, a fixed-length feature vector per image whatever its
    size: region (i, j) holds the patches whose start-row index is in ``pool_regions(nr, gh)[i]`` and whose start-column
    index is in ``pool_regions(nc, gw)[j]``.  ``reduce`` is ``'mean'``, ``'sum'`` or ``'max'`` (``pool_codes``; validated
    always, read only with ``pool``).  The maps themselves are then never held: every chunk's codes are pooled on the device
    (pm_codes_pool_f64) in an order that is the same for every chunking.

    It inherits from ``encode()``: this rank's images only, no collective; the training state, ``model_params`` and Hprime /
    gamma are left as they were.  A NaN pixel makes NaN exactly the map cells of the patches that contain it, and exactly the
    regions that contain those.  NumPy arrays, or with ``device=True`` ``DeviceArray``s."""
    from ..em.camodels._device import DeviceArray
    if mask is not None and center:
        raise ValueError("center=True with a mask is not built: the patch mean would have to run over the observed pixels only")
    if weight is not None and mask is not None:
        raise ValueError("'weight' together with 'mask': fold the mask into the weight as zeros (weight = 0 where mask == 0)")
    if weight is not None and center:
        raise ValueError("center=True with a weight is not built: the patch mean would have to be the weighted one")
    _reduce_check(reduce)
    D, H = int(model.D), int(model.H)
    if patch is None:
        p = int(round(D ** 0.5))
        if p * p != D:
            raise ValueError("model.D = %d is not a square: give patch=(p_h, p_w)" % D)
        patch = (p, p)
    ph, pw = _patch_pair(patch)
    if ph * pw != D:
        raise ValueError("a %d x %d patch has %d values, model.D is %d" % (ph, pw, ph * pw, D))
    shape = _shape_of(image)
    geo = _geometry(shape, (ph, pw), stride)
    (B, Hi, Wi), _, _, nr, nc = geo
    if chunk is None:
        chunk = CHUNK_BYTES // (8 * (D + 2 * H))
    elif int(chunk) != chunk or int(chunk) < 1:
        raise ValueError("chunk must be a positive number of patches, got %r" % (chunk,))
    rows = min(max(1, int(chunk) // nc), B * nr)
    if pool is not None:
        pool = _pool_pair(pool, nr, nc)
    extra = {'exact': True} if exact else {}
    if mask is not None:
        if _shape_of(mask) != tuple(shape):
            raise ValueError("mask has shape %r, the image %r" % (_shape_of(mask), tuple(shape)))
        # (an empty masked call: a model without the masked E-step refuses here, before anything reaches the device)
        model.encode(model_params, {'y': np.empty((0, D)), 'mask': np.empty((0, D), dtype=bool)}, **extra)
    if weight is not None:
        if _shape_of(weight) != tuple(shape):
            raise ValueError("weight has shape %r, the image %r" % (_shape_of(weight), tuple(shape)))
        _weight_check(weight)
        # (an empty weighted call: a model without the weighted E-step refuses here, before anything reaches the device)
        model.encode(model_params, {'y': np.empty((0, D)), 'weight': np.empty((0, D))}, **extra)
    dev = _device(model)
    det = bool(getattr(model, "deterministic", False))
    img, ldi = _image_tensor(image, dev)
    mimg, ldmi = _mask_image(mask, shape, dev) if mask is not None else (None, 0)
    wimg, ldwi = _weight_image(weight, dev) if weight is not None else (None, 0)
    grid, N = (B, nr, nc), B * nr * nc
    if pool is None:
        outs = [torch.empty((N, H), dtype=torch.float64, device=dev) for _ in range(2)]
    else:
        outs = [_pool_begin(grid, pool, H, reduce, dev) for _ in range(2)]
        work = _pool_work(rows, nc, pool[1], H, dev)
    for R0 in range(0, B * nr, rows):
        n0, n = R0 * nc, min(rows, B * nr - R0) * nc
        Y, _ = _extract(img, ldi, geo, n0, n, center, det)
        data = {'y': DeviceArray(Y)}
        if mimg is not None:
            data['mask'] = DeviceArray((_extract(mimg, ldmi, geo, n0, n, False, det)[0] != 0).view(torch.uint8))
        if wimg is not None:
            data['weight'] = DeviceArray(_extract(wimg, ldwi, geo, n0, n, False, det)[0])
        pair = model.encode(model_params, data, device=True, **extra)
        del Y, data
        for out, code, what in zip(outs, pair, ("mean", "prob")):
            if _shape_of(code) != (n, H):
                raise ValueError("encode() returned a %s of %r for a chunk of (%d, %d)" % (what, _shape_of(code), n, H))
            code, ldc = _rows_tensor(code, H, dev, "encode()'s %s" % what)
            if pool is None:
                out[n0:n0 + n].copy_(code)
            else:
                _pool(out, code, ldc, grid, pool, n0, n, reduce, work, det)
        del pair, code
    if pool is None:
        outs = [t.view(B, nr, nc, H) for t in outs]
    else:
        outs = [_pool_finish(t, grid, pool, reduce, det) for t in outs]
    return tuple(_hand_back(t, len(shape) == 2, device) for t in outs)
