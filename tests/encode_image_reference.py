"""The pooling of encode_image() / pool_codes() stated in plain Python floats, in exactly the order the header
(include/prosper_hip.h, pm_codes_pool_f64) fixes: what the GPU tests compare against bit for bit.  Pinned on the CPU by
tests/test_encode_image_cpu.py.

The patches of a grid (B, nr, nc) are numbered row-major over (image, start row, start column); ``codes`` is (B nr nc, H)."""
import math

import numpy as np


def pool_regions(n, g):
    """Region i of an axis of n patch positions cut into g: [floor(i n / g), floor((i + 1) n / g))."""
    if not 1 <= g <= n:
        raise ValueError("1 <= g <= n, got n = %r, g = %r" % (n, g))
    return [(i * n // g, (i + 1) * n // g) for i in range(g)]


def larger(a, x):
    """The larger of two floats by explicit compares: a NaN on either side is the result, max(-0, +0) = +0."""
    if a != a:
        return a
    if x != x:
        return x
    if x > a or (x == a and math.copysign(1.0, x) > 0):
        return x
    return a


def pool(codes, grid, pool, reduce="sum", reverse=False):
    """(B, gh, gw, H) float64.  sum: acc <- acc + t_R over the patch rows R of the region in ascending order, acc starting at
    +0, t_R = (((+0 + x[R, c0]) + x[R, c0 + 1]) + ...) over the region's columns in ascending order.  mean: that sum divided
    once by rows x columns.  max: the same walk with ``larger`` from -inf.  ``reverse=True`` walks rows and columns in
    descending order instead: only there to show that a test can see the order."""
    B, nr, nc = grid
    gh, gw = pool
    codes = np.asarray(codes, dtype=np.float64)
    N, H = codes.shape
    assert N == B * nr * nc and reduce in ("sum", "mean", "max")
    x = codes.reshape(B, nr, nc, H).tolist()
    step = (lambda a, v: a + v) if reduce != "max" else larger
    unit = 0.0 if reduce != "max" else -math.inf
    out = np.empty((B, gh, gw, H))
    for b in range(B):
        for i, (r0, r1) in enumerate(pool_regions(nr, gh)):
            rows = range(r0, r1)[::-1] if reverse else range(r0, r1)
            for j, (c0, c1) in enumerate(pool_regions(nc, gw)):
                cols = range(c0, c1)[::-1] if reverse else range(c0, c1)
                for h in range(H):
                    acc = unit
                    for r in rows:
                        t = unit
                        row = x[b][r]
                        for c in cols:
                            t = step(t, row[c][h])
                        acc = step(acc, t)
                    out[b, i, j, h] = acc / ((r1 - r0) * (c1 - c0)) if reduce == "mean" else acc
    return out


def wide_range(rng, shape):
    """normal * 10^uniform(-8, 8): sums of such values round differently in different orders."""
    return rng.normal(size=shape) * 10.0 ** rng.uniform(-8, 8, size=shape)


def same_bits(got, want, what=""):
    """Bit equality of two float64 arrays; NaNs must sit in the same places (their payloads are not compared)."""
    got, want = np.ascontiguousarray(np.asarray(got)), np.ascontiguousarray(np.asarray(want, dtype=np.float64))
    assert got.shape == want.shape and got.dtype == np.float64, (what, got.shape, want.shape, got.dtype)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "%s: NaNs in different places (%d against %d)" % (what, gn.sum(), wn.sum())
    diff = (got.view(np.uint64) != want.view(np.uint64)) & ~gn
    assert not diff.any(), "%s: %d of %d values differ, first at %s" % (what, diff.sum(), diff.size, np.argwhere(diff)[:1])
