#!/usr/bin/env python3
"""Extract, encode, pool: a learned dictionary as a feature extractor for whole images.

    python examples/encode_image.py [bsc|mca] [--size 24] [--p 5] [--train 40] [--test 100] [--steps 40] [--pool 2]
                                    [--reduce mean|sum|max] [--stride 1]

No file is read.  Two classes of *bars images*: class 0 holds horizontal bars only (row indicators r_i ~ Bernoulli(pi),
clean[i, j] = a r_i), class 1 vertical bars only (clean[i, j] = a c_j); both get Gaussian noise of standard deviation sigma.
The two classes have the same pixel statistics -- the mean image of either is the constant a pi -- so a classifier on raw
pixels has nothing to hold on to, while the p x p patches of either class are datapoints of the bars model with H = 2p (p
horizontal and p vertical bars), whose latents say which orientation is there.

The model is trained on the patches of a mixed training set (``extract_patches`` of the stack, handed to EM on the device).
Then every image goes through ``encode_image(..., pool=g)``: the posterior activation probabilities of its patches, pooled
over a g x g grid of regions into a vector of g g H features.  A nearest-centroid classifier on those vectors is scored on a
held-out test set, beside the same classifier on the raw pixels."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from prosper_amd.em import EM                                  # noqa: E402
from prosper_amd.em.annealing import LinearAnnealing           # noqa: E402
from prosper_amd.utils.patches import extract_patches          # noqa: E402


def bars_images(rng, n, size, a, pi, sigma):
    """(2n, size, size) noisy images and their labels: n with horizontal bars only, then n with vertical bars only."""
    on = rng.uniform(size=(2 * n, size)) < pi
    clean = np.empty((2 * n, size, size))
    clean[:n] = a * on[:n, :, None]
    clean[n:] = a * on[n:, None, :]
    return clean + sigma * rng.normal(size=clean.shape), np.repeat([0, 1], n)


def build(name, p, Hprime, gamma):
    if name == "mca":
        from prosper_amd.em.camodels.mca_et import MCA_ET as Model
    else:
        from prosper_amd.em.camodels.bsc_et import BSC_ET as Model
    return Model(p * p, 2 * p, Hprime, gamma)


def nearest_centroid(train, train_labels, test, test_labels):
    """Accuracy on ``test`` of the classifier that assigns the class whose training mean is nearest (Euclidean)."""
    train, test = train.reshape(len(train), -1), test.reshape(len(test), -1)
    centroids = np.stack([train[train_labels == k].mean(axis=0) for k in (0, 1)])
    dist = ((test[:, None, :] - centroids[None, :, :]) ** 2).sum(axis=2)
    return float((dist.argmin(axis=1) == test_labels).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("model", nargs="?", default="bsc", choices=["bsc", "mca"])
    ap.add_argument("--size", type=int, default=24, help="the images are size x size")
    ap.add_argument("--p", type=int, default=5, help="patch side; H = 2p")
    ap.add_argument("--stride", type=int, default=1)
    ap.add_argument("--train", type=int, default=40, help="training images per class")
    ap.add_argument("--test", type=int, default=100, help="test images per class")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--pool", type=int, default=2, help="the features are pooled over a pool x pool grid of regions")
    ap.add_argument("--reduce", default="mean", choices=["mean", "sum", "max"])
    ap.add_argument("--a", type=float, default=5.0, help="height of a bar")
    ap.add_argument("--sigma", type=float, default=1.0)
    ap.add_argument("--pi", type=float, default=0.2)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    np.random.seed(a.seed)
    rng = np.random.RandomState(a.seed)
    train, train_labels = bars_images(rng, a.train, a.size, a.a, a.pi, a.sigma)
    test, test_labels = bars_images(rng, a.test, a.size, a.a, a.pi, a.sigma)
    H = 2 * a.p

    # train on the patches of the mixed training set: the (N, D) matrix never exists on the host
    model = build(a.model, a.p, min(H, 5), min(H, 3))
    anneal = LinearAnnealing(a.steps)
    anneal['T'] = [(0, 2.), (.7, 1.)]
    anneal['Ncut_factor'] = [(0, 0.), (2. / 3, 1.)]
    anneal['anneal_prior'] = False
    Y, _ = extract_patches(train, a.p, stride=1, device=True)
    em = EM(model=model, anneal=anneal, data={'y': Y}, lparams=model.standard_init({'y': Y}))
    em.run()
    learned = dict(em.lparams)

    # encode over a wider truncated state set than training uses (as examples/denoise_image.py), pool, classify
    emodel = build(a.model, a.p, min(H, 7), min(H, 5))
    kw = dict(stride=a.stride, pool=a.pool, reduce=a.reduce)
    _, f_train = emodel.encode_image(learned, train, **kw)
    _, f_test = emodel.encode_image(learned, test, **kw)
    print("%s, two classes of %d x %d bars images (a = %g, sigma = %g, pi = %g): horizontal bars only / vertical bars only"
          % (a.model.upper(), a.size, a.size, a.a, a.sigma, a.pi))
    print("  %d x %d patches, H = %d, %d patches of %d training images trained on, %d EM steps"
          % (a.p, a.p, H, len(Y), len(train), a.steps))
    print("  features: prob of encode_image(pool=%d, reduce='%s', stride=%d), %d numbers per image (raw pixels: %d)"
          % (a.pool, a.reduce, a.stride, f_train[0].size, a.size * a.size))
    print("  nearest-centroid test accuracy on %d images: pooled codes %.3f   raw pixels %.3f"
          % (len(test), nearest_centroid(f_train, train_labels, f_test, test_labels),
             nearest_centroid(train, train_labels, test, test_labels)))
    print("  learned pi %.4f (generating %.4f: a patch holds bars of one orientation only), sigma %.4f (generating %.4f)"
          % (float(np.asarray(learned['pi'])), a.pi / 2, float(np.asarray(learned['sigma'])), a.sigma))


if __name__ == "__main__":
    main()
