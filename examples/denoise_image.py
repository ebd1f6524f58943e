#!/usr/bin/env python3
"""Whole-image denoising by overlapping patches on an image the models are correctly specified for.

    python examples/denoise_image.py [bsc|mca] [--size 128] [--p 5] [--stride 1] [--steps 50] [--missing FRACTION]
                                     [--train-missing] [--variance] [--aggregate precision [--floor F ...]]
                                     [--noise-ramp R]

No file is read.  The script draws a *bars image*: row indicators r_i and column indicators c_j ~ Bernoulli(pi),
clean[i, j] = a (r_i + c_j) (MCA: a max(r_i, c_j)), plus Gaussian noise of standard deviation sigma.  Every p x p patch of
that image is a datapoint of the bars model with H = 2p (p horizontal and p vertical bars of height a), so the model is
correctly specified for every overlapping patch.  The model is trained on the noisy image's own patches -- extracted on the
device and handed to EM as they are, with the annealing schedule of examples/bars_learning.py -- and the image is denoised
with ``reconstruct_image`` at the learned and at the generating parameters; noisy and denoised MSE / PSNR are printed.

``--missing FRACTION`` (missing values): after the noise that share of the pixels is dropped at random.  The
model trains on the complete noisy image, the reconstruction runs with the mask (``reconstruct_image(..., mask=)``; the
dropped pixels hold NaN), and the MSE is printed separately over the observed pixels (denoising) and over the missing ones
(inpainting, next to filling them with the observed pixels' mean).

``--train-missing`` (``bsc`` with ``--missing``): nobody has the complete image -- the model trains on the
incomplete image's own patches.  The mask image goes through ``extract_patches`` on the same grid and travels as
``my_data['mask']`` through EM; ``Ncut_factor`` stays 0 (data truncation is not defined across rows with different numbers
of observed pixels); the start parameters come from the image with its holes filled by the observed mean.  The same
observed / missing MSE lines are printed.

``--variance``: ``reconstruct_image(..., variance=True)`` also returns ``var_map``, the overlap average of the
patches' posterior variances of the noiseless value -- an upper bound on the variance of the averaged estimate.  Its mean is
printed beside the actual MSE against the clean image (with ``--missing``: separately over the observed and over the missing
pixels).

``--aggregate precision``: beside the plain overlap average the image is also aggregated with every patch's
estimate of a pixel weighted by 1 / (V + floor), V its posterior variance (``reconstruct_image(..., aggregate='precision')``);
MSE and PSNR of both are printed side by side, with ``--missing`` over the observed, the missing and all pixels.  ``--floor F
...``: the floor(s) to run instead of the default (``utils.patches.PRECISION_FLOOR`` times the model's noise variance).

``--noise-ramp R`` (per-pixel noise weights): the noise standard deviation rises linearly from the left edge to
the right edge by the factor R, scaled so that the mean noise variance stays sigma^2.  The model trains as before (it learns one
sigma), and the image is denoised twice: without weights, and with ``reconstruct_image(..., weight=)`` at weight = mean noise
variance / pixel noise variance; MSE and PSNR of both are printed side by side.  Composes with ``--aggregate precision`` and
``--variance``; not with ``--missing``."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from prosper_amd.em import EM                                  # noqa: E402
from prosper_amd.em.annealing import LinearAnnealing           # noqa: E402
from prosper_amd.utils.patches import extract_patches          # noqa: E402


def bars_image(rng, size, a, pi, sigma, mca):
    r, c = rng.uniform(size=size) < pi, rng.uniform(size=size) < pi
    clean = a * (np.maximum(r[:, None], c[None, :]) if mca else r[:, None].astype(float) + c[None, :]).astype(np.float64)
    return clean, clean + sigma * rng.normal(size=(size, size))


def bars_dict(p, a):
    """(p^2, 2p): p horizontal, then p vertical bars of height a."""
    W = np.zeros((p, p, 2 * p))
    for h in range(p):
        W[h, :, h] = a
        W[:, h, p + h] = a
    return W.reshape(p * p, 2 * p)


def build(name, p, Hprime, gamma):
    if name == "mca":
        from prosper_amd.em.camodels.mca_et import MCA_ET as Model
    else:
        from prosper_amd.em.camodels.bsc_et import BSC_ET as Model
    return Model(p * p, 2 * p, Hprime, gamma)


def report(tag, img, clean, peak):
    mse = float(((np.asarray(img) - clean) ** 2).mean())
    print("  %-44s MSE %.4f   PSNR %.2f dB" % (tag, mse, 10 * np.log10(peak ** 2 / mse)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("model", nargs="?", default="bsc", choices=["bsc", "mca"])
    ap.add_argument("--size", type=int, default=128, help="the image is size x size")
    ap.add_argument("--p", type=int, default=5, help="patch side; H = 2p")
    ap.add_argument("--stride", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--a", type=float, default=5.0, help="height of a bar")
    ap.add_argument("--sigma", type=float, default=1.0)
    ap.add_argument("--pi", type=float, default=0.2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--missing", type=float, default=0.0, metavar="FRACTION",
                    help="share of pixels dropped after the noise; the reconstruction runs with the mask")
    ap.add_argument("--train-missing", action="store_true",
                    help="bsc with --missing: train on the incomplete image's own patches (my_data['mask'])")
    ap.add_argument("--variance", action="store_true",
                    help="also print the mean of var_map (the posterior variance the model reports) beside the MSE")
    ap.add_argument("--aggregate", default="mean", choices=["mean", "precision"],
                    help="precision: also aggregate with the estimates weighted by 1 / (V + floor) and print both")
    ap.add_argument("--floor", type=float, nargs="+", default=None, metavar="F",
                    help="with --aggregate precision: the floor(s) to use (default: PRECISION_FLOOR x the noise variance)")
    ap.add_argument("--noise-ramp", type=float, default=None, metavar="R",
                    help="noise standard deviation rising linearly left to right by the factor R; denoise without and with "
                         "the weight image mean noise variance / pixel noise variance")
    a = ap.parse_args()
    if a.noise_ramp is not None and (a.missing > 0.0 or a.train_missing or not a.noise_ramp > 0.0):
        ap.error("--noise-ramp needs R > 0 and does not combine with --missing")
    if a.floor is not None and a.aggregate != "precision":
        ap.error("--floor needs --aggregate precision")
    if a.train_missing and (a.model != "bsc" or not 0.0 < a.missing < 1.0):
        ap.error("--train-missing needs the bsc model and --missing FRACTION in (0, 1)")
    np.random.seed(a.seed)
    rng = np.random.RandomState(a.seed)
    mca = a.model == "mca"
    clean, noisy = bars_image(rng, a.size, a.a, a.pi, a.sigma, mca)
    weight = None
    if a.noise_ramp is not None:
        # sd(column j) = s0 (1 + (R - 1) j / (size - 1)), s0 so that the mean noise variance is sigma^2
        ramp = 1.0 + (a.noise_ramp - 1.0) * np.arange(a.size) / max(a.size - 1, 1)
        sd = np.tile((a.sigma * ramp / np.sqrt((ramp ** 2).mean()))[None, :], (a.size, 1))
        noisy = clean + sd * rng.normal(size=clean.shape)
        weight = (sd ** 2).mean() / sd ** 2
    H = 2 * a.p
    gt = {'W': bars_dict(a.p, a.a), 'pi': a.pi, 'sigma': a.sigma}

    # train on the noisy image's own patches: the (N, D) matrix never exists on the host
    model = build(a.model, a.p, min(H, 5), min(H, 3))
    anneal = LinearAnnealing(a.steps)
    anneal['T'] = [(0, 2.), (.7, 1.)]
    anneal['anneal_prior'] = False
    mask = None
    if a.train_missing:
        # ... of the INCOMPLETE image: the mask image's patches on the same grid are the patches' masks
        mask = rng.uniform(size=clean.shape) >= a.missing
        holes = np.where(mask, noisy, np.nan)
        Y, _ = extract_patches(holes, a.p, stride=1, device=True)
        Mp, _ = extract_patches(mask.astype(np.float64), a.p, stride=1, device=True)
        filled, _ = extract_patches(np.where(mask, noisy, noisy[mask].mean()), a.p, stride=1, device=True)
        init = model.standard_init({'y': filled})
        data = {'y': Y, 'mask': Mp}
    else:
        Y, _ = extract_patches(noisy, a.p, stride=1, device=True)
        init = model.standard_init({'y': Y})
        anneal['Ncut_factor'] = [(0, 0.), (2. / 3, 1.)]
        data = {'y': Y}
    em = EM(model=model, anneal=anneal, data=data, lparams=init)
    em.run()
    learned = dict(em.lparams)

    # denoise over a wider truncated state set than training uses (as examples/bars_learning.py --reconstruct)
    rmodel = build(a.model, a.p, min(H, 7), min(H, 5))
    peak = float(clean.max()) or 1.0
    kw = {'variance': True} if a.variance else {}
    psnr = lambda m: 10 * np.log10(peak ** 2 / m)

    def aggregates(params):
        """[(label, keywords)]: the plain average, then the precision aggregate at every floor asked for."""
        runs = [("", {})]
        if a.aggregate == "precision":
            from prosper_amd.utils.patches import PRECISION_FLOOR
            for f in a.floor or [None]:
                used = PRECISION_FLOOR * rmodel._noise_variance(params) if f is None else f
                runs.append((", precision (floor %.4g)" % used, {'aggregate': 'precision', 'floor': f}))
            runs[0] = (", mean", {})
        return runs
    print("%s, %d x %d bars image (a = %g, sigma = %g, pi = %g), %d x %d patches at stride %d, %d patches trained on, %d EM steps"
          % (a.model.upper(), a.size, a.size, a.a, a.sigma, a.pi, a.p, a.p, a.stride, len(Y), a.steps))
    if a.missing > 0.0:
        if not a.missing < 1.0:
            ap.error("--missing is a fraction in [0, 1)")
        if mask is None:
            mask = rng.uniform(size=clean.shape) >= a.missing
        holes = np.where(mask, noisy, np.nan)
        print("  %.1f %% of the pixels dropped after the noise; trained on the %s" % (
            100 * (1 - mask.mean()), "incomplete image's own patches (%d dimensions of W kept their row in the last step)"
            % model.W_kept if a.train_missing else "complete noisy image"))
        mse = lambda img, sel: float(((np.asarray(img) - clean)[sel] ** 2).mean())
        print("  %-44s MSE observed %.4f   missing %.4f (filled with the observed mean)"
              % ("noisy image", mse(noisy, mask), mse(np.full_like(clean, noisy[mask].mean()), ~mask)))
        for tag, params in (("learned", learned), ("generating", gt)):
            base = None
            for label, agg in aggregates(params):
                out = rmodel.reconstruct_image(params, holes, mask=mask, stride=a.stride, **dict(kw, **agg))
                out, var = out if a.variance else (out, None)
                line = "  %-44s MSE observed %.4f   missing %.4f" % ("reconstructed, %s%s" % (tag, label or " parameters"),
                                                                     mse(out, mask), mse(out, ~mask))
                if a.aggregate == "precision":
                    everything = mse(out, np.ones_like(mask))
                    line += "   all %.4f   PSNR %.2f dB" % (everything, psnr(everything))
                    line += "" if base is None else " (%+.3f dB)" % (psnr(everything) - base)
                    base = psnr(everything) if base is None else base
                print(line)
                if a.variance:
                    print("  %-44s     observed %.4f   missing %.4f" % ("  mean of var_map", var[mask].mean(), var[~mask].mean()))
        return
    report("noisy image", noisy, clean, peak)
    if weight is not None:
        print("  noise ramp %g: pixel noise standard deviation %.4f (left) to %.4f (right), weights %.4f to %.4f"
              % (a.noise_ramp, sd[0, 0], sd[0, -1], weight.max(), weight.min()))
    runs = [("", {})] if weight is None else [(", no weights", {}), (", weighted", {'weight': weight})]
    for tag, params in (("learned", learned), ("generating", gt)):
        for wlabel, wkw in runs:
            base = None
            for label, agg in aggregates(params):
                out = rmodel.reconstruct_image(params, noisy, stride=a.stride, **dict(kw, **dict(agg, **wkw)))
                out, var = out if a.variance else (out, None)
                report("denoised, %s%s%s" % (tag, wlabel, label or ("" if wlabel else " parameters")), out, clean, peak)
                if a.aggregate == "precision":
                    now = psnr(float(((np.asarray(out) - clean) ** 2).mean()))
                    if base is not None:
                        print("  %-44s %+.3f dB against the mean aggregate" % ("", now - base))
                    base = now if base is None else base
                if a.variance:
                    print("  %-44s     %.4f (mean of var_map: the posterior variance the model reports)" % ("", var.mean()))
    print("  learned pi %.4f (generating %.4f), sigma %.4f (generating %.4f)"
          % (float(np.asarray(learned['pi'])), a.pi, float(np.asarray(learned['sigma'])), a.sigma))


if __name__ == "__main__":
    main()
