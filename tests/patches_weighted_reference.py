"""NumPy statement of the weighted overlap average, shared by tests/test_patches_weighted_cpu.py and
tests/test_patches_weighted_gpu.py: explicit loops over the patches in ascending patch number, over a patch's rows and over
its elements, every step one ``np.float64`` operation -- one IEEE rounding -- so that the device kernel can be held to its
bits.  The grid comes from tests/patches_reference.py.  Not a test module."""
import numpy as np

import patches_reference as P

F = np.float64


def weight(wgt_ke, wmode, floor, window_e):
    """w = a b of one patch element; a factor that is not there (None) is not multiplied."""
    a = None
    if wgt_ke is not None:
        a = F(wgt_ke)
        if wmode == 1:
            v = F(0.0) if a < F(0.0) else a            # (a NaN is not < 0: it stays)
            a = F(1.0) / (v + F(floor))
    if window_e is None:
        return F(1.0) if a is None else a
    return F(window_e) if a is None else a * F(window_e)


def accumulate(num, den, est, shape, patch, stride, wgt=None, wmode=0, floor=0.0, window=None, means=None, n0=0, n=None):
    """num (B, Hi, Wi) <- num + (w t), den <- den + w (den None: skipped) over the patches [n0, n0 + n) in ascending number;
    ``est`` / ``wgt`` / ``means`` are indexed by the patch number itself.  In place; returns (num, den)."""
    full = (1,) + tuple(shape) if len(shape) == 2 else tuple(shape)
    ph, pw = patch
    g = P.grid(full, patch, stride)
    n = len(g) - n0 if n is None else n
    with np.errstate(all="ignore"):
        for k in range(n0, n0 + n):
            b, i, j = g[k]
            for a_ in range(ph):
                for b_ in range(pw):
                    e = a_ * pw + b_
                    w = weight(None if wgt is None else wgt[k, e], wmode, floor, None if window is None else window[e])
                    t = F(est[k, e])
                    if means is not None:
                        t = t + F(means[k])
                    prod = w * t
                    num[b, i + a_, j + b_] = num[b, i + a_, j + b_] + prod
                    if den is not None:
                        den[b, i + a_, j + b_] = den[b, i + a_, j + b_] + w
    return num, den


def finish(num, den):
    """num / den, one IEEE division per pixel; 0 / 0 is NaN."""
    with np.errstate(all="ignore"):
        return np.asarray(num, dtype=F) / np.asarray(den, dtype=F)


def average(est, shape, patch, stride, wgt=None, wmode=0, floor=0.0, window=None, means=None):
    """The weighted average of a whole patch matrix from zeroed sums, in the shape of ``shape``."""
    full = (1,) + tuple(shape) if len(shape) == 2 else tuple(shape)
    num, den = np.zeros(full, dtype=F), np.zeros(full, dtype=F)
    accumulate(num, den, est, shape, patch, stride, wgt, wmode, floor, None if window is None else np.asarray(window, F).reshape(-1),
               means)
    return finish(num, den).reshape(shape)


def weighted_variance(V, shape, patch, stride, floor, window=None):
    """var_map of aggregate='precision': sum (w V) / sum w with w = 1 / (max(V, 0) + floor) (times the window)."""
    return average(V, shape, patch, stride, wgt=V, wmode=1, floor=floor, window=window)
