"""NumPy statement of the patch grid, patch extraction and the overlap average, shared by
tests/test_patches_cpu.py and tests/test_patches_gpu.py: plain loops over the patches in patch order.  Not a test module."""
import numpy as np


def starts(L, p, s):
    """0, s, 2s, ... while start + p <= L, plus L - p if the last of them is not L - p."""
    out = []
    x = 0
    while x + p <= L:
        out.append(x)
        x += s
    if out[-1] != L - p:
        out.append(L - p)
    return out


def _stack(img):
    img = np.asarray(img)
    return img[None] if img.ndim == 2 else img


def grid(shape, patch, stride):
    """[(image, start row, start column)] in patch order."""
    B, Hi, Wi = (1,) + tuple(shape) if len(shape) == 2 else tuple(shape)
    ph, pw = patch
    return [(b, i, j) for b in range(B) for i in starts(Hi, ph, stride) for j in starts(Wi, pw, stride)]


def extract(img, patch, stride):
    """(N, D) float64: patch k, row-major values."""
    img = _stack(img)
    ph, pw = patch
    return np.array([img[b, i:i + ph, j:j + pw].astype(np.float64).reshape(-1) for b, i, j in grid(img.shape, patch, stride)])


def cover(shape, patch, stride):
    """Number of patches that contain each pixel, (B, Hi, Wi) int64."""
    B, Hi, Wi = (1,) + tuple(shape) if len(shape) == 2 else tuple(shape)
    ph, pw = patch
    cnt = np.zeros((B, Hi, Wi), dtype=np.int64)
    for b, i, j in grid((B, Hi, Wi), patch, stride):
        cnt[b, i:i + ph, j:j + pw] += 1
    return cnt


def average(P, shape, patch, stride, means=None):
    """acc[i:i+p, j:j+p] = acc[...] + (P[k] + mean_k) over the patches in patch order, then acc / count."""
    full = (1,) + tuple(shape) if len(shape) == 2 else tuple(shape)
    ph, pw = patch
    acc = np.zeros(full, dtype=np.float64)
    P = np.asarray(P, dtype=np.float64)
    for k, (b, i, j) in enumerate(grid(full, patch, stride)):
        v = P[k].reshape(ph, pw)
        if means is not None:
            v = v + means[k]
        acc[b, i:i + ph, j:j + pw] = acc[b, i:i + ph, j:j + pw] + v
    out = acc / cover(full, patch, stride)
    return out[0] if len(shape) == 2 else out


def patches_containing(shape, patch, stride, pixel):
    """Boolean (Hi, Wi) mask: the union of the patches of a single image that contain ``pixel`` = (i, j)."""
    Hi, Wi = shape
    ph, pw = patch
    mask = np.zeros((Hi, Wi), dtype=bool)
    for _, i, j in grid((Hi, Wi), patch, stride):
        if i <= pixel[0] < i + ph and j <= pixel[1] < j + pw:
            mask[i:i + ph, j:j + pw] = True
    return mask


def bars_image(rng, Hi, Wi, a, pi, sigma, mca=False):
    """(clean, noisy, r, c): row / column indicators ~ Bernoulli(pi), clean[i, j] = a (r_i + c_j) (MCA: a max(r_i, c_j)),
    noisy = clean + N(0, sigma^2)."""
    r = rng.uniform(size=Hi) < pi
    c = rng.uniform(size=Wi) < pi
    clean = a * (np.maximum(r[:, None], c[None, :]) if mca else (r[:, None].astype(float) + c[None, :]))
    clean = clean.astype(np.float64)
    return clean, clean + sigma * rng.normal(size=(Hi, Wi)), r, c


def bars_W(p, a):
    """(p*p, 2p): the generating dictionary of the p x p patches of a bars image -- p horizontal, then p vertical bars."""
    W = np.zeros((p * p, 2 * p))
    for h in range(p):
        m = np.zeros((p, p))
        m[h, :] = a
        W[:, h] = m.reshape(-1)
        m = np.zeros((p, p))
        m[:, h] = a
        W[:, p + h] = m.reshape(-1)
    return W
