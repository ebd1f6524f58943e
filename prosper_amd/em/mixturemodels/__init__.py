"""Mixture-model base: restates prosper/em/mixturemodels/__init__.py (``MixtureModel`` :28-153).

``MoG`` and ``MoP`` supply ``E_step`` / ``M_step``; in this package both run as HIP kernels on the MI355X
(``_device``).  Host-side behaviour -- initialisation, data generation, row subsets, logging -- follows the reference
draw for draw; where the reference cannot run as written the docstring says what is done instead.
"""
import numpy as np
from scipy import stats

from .. import Model
from ...utils import parallel
from ...utils import tracing
from ...utils.datalog import dlog


def _host(y):
    """A data shard as a host float64 array (``DeviceArray`` handles and tensors download once)."""
    if hasattr(y, "numpy") and not isinstance(y, np.ndarray):
        y = y.numpy() if not hasattr(y, "detach") else y.detach().cpu().numpy()
    return np.asarray(y, dtype=np.float64)


class MixtureModel(Model):
    """Abstract mixture model over H components of D-dimensional data."""

    def __init__(self, D, H, to_learn=['W', 'pies'], comm=parallel.COMM_WORLD):
        Model.__init__(self, comm)
        self.to_learn = to_learn
        self.D = D
        self.H = H

    @tracing.traced
    def standard_init(self, data):
        """W = the collective data mean + N(0, (sigma_init / 4)^2) noise, pies = 1/H (__init__.py:41-74).

        The RNG order is the reference's: one ``np.random.normal(scale=noise, size=[D, H])``.  ``sigma_init`` is the
        mean over dimensions of the square root of the collective per-dimension variance around that mean."""
        comm = self.comm
        H = self.H
        my_y = _host(data['y'])
        my_N, D = my_y.shape
        assert D == self.D
        W_mean = parallel.allmean(my_y, axis=0, comm=comm)
        sigma_sq = parallel.allmean((my_y - W_mean) ** 2, axis=0, comm=comm)
        sigma_init = np.sqrt(sigma_sq).sum() / D
        noise = sigma_init / 4.
        W_init = W_mean[:, None] + np.random.normal(scale=noise, size=[D, H])
        model_params = {'W': W_init}
        if 'pies' in self.to_learn:
            model_params['pies'] = np.ones(H) * 1. / H
        return model_params

    @tracing.traced
    def kmeanspp_init(self, data, seed=None, uniforms=None):
        """k-means++ seeding in place of ``standard_init``'s H coincident components: W (D, H) holds H
        datapoints drawn by D^2 sampling on the device (``utils.seeding.kmeanspp``: squared Euclidean distance for every
        model; ``seed`` / ``uniforms`` as there and as in ``sample_posterior``), pies = 1/H when learned, and every other entry
        is what ``standard_init`` puts there, from the same code (MoG: the shared covariance) -- the two inits differ in W
        alone.  No NumPy random number is drawn.  The dict goes through ``check_params`` and is broadcast like
        ``standard_init``'s.  ``self.seed_indices`` (H,) are the global row numbers of the chosen datapoints and
        ``self.seed_potential`` (H,) the seeding potential after each of them.  MoP: W = max(datapoint, eps) -- a zero count
        would be a zero rate, whose logarithm the E-step cannot weigh; eps is the floor its M-step keeps W above.

        Collective.  ``ValueError`` as ``kmeanspp`` raises them, and for data whose second axis is not D -- before any
        launch; fewer than H distinct rows and non-finite data after the rounds."""
        from ...utils.seeding import kmeanspp
        y = data['y']
        shape = tuple(getattr(y, "tensor", y).shape)
        if len(shape) != 2 or shape[1] != self.D:
            raise ValueError("%s.kmeanspp_init: data['y'] must be (my_N, %d), got %r" % (type(self).__name__, self.D, shape))
        import contextlib
        import torch
        # (a model bound to a device runs there; otherwise the current device, looked up after kmeanspp's refusals)
        with torch.cuda.device(self._device) if self._device is not None else contextlib.nullcontext():
            centres, indices, potential = kmeanspp(y, self.H, seed=seed, uniforms=uniforms, comm=self.comm,
                                                   deterministic=bool(getattr(self, "deterministic", False)))
        self.seed_indices, self.seed_potential = indices, potential
        model_params = {'W': self._seed_rates(np.ascontiguousarray(centres.T))}
        if 'pies' in self.to_learn:
            model_params['pies'] = np.ones(self.H) * 1. / self.H
        model_params = self._init_noise(model_params, data)
        return self.comm.bcast(self.check_params(model_params))

    def _seed_rates(self, W):
        """What a model makes of the chosen datapoints before they become W (MoP: rates are positive)."""
        return W

    def _init_noise(self, model_params, data):
        """The entries of an initial parameter dict beside W and pies (MoG: sigmas_sq); shared by both inits."""
        return model_params

    def check_params(self, model_params):
        raise NotImplementedError

    def _noise_variance(self, model_params):
        """The noise variance ``reconstruct_image(aggregate='precision')`` scales its default floor by; a model without a
        noise parameter (MoP) has none."""
        raise ValueError("%s has no noise parameter to derive the precision floor from: give floor=" % type(self).__name__)

    def reconstruct_image(self, model_params, image, mask=None, weight=None, **kw):
        """Whole-image denoising by overlapping patches: ``utils.patches.denoise_image(self, model_params,
        image, **kw)`` -- every patch through ``reconstruct()``, the estimates averaged where they overlap.  Keywords:
        ``patch``, ``stride``, ``center``, ``chunk``, ``device``, ``exact`` (every patch through
        ``reconstruct(exact=True)``), ``variance`` (returns ``(image, var_map)``, var_map the overlap average of
        the patches' posterior variances -- an upper bound on the variance of the averaged estimate).  ``mask`` (the image's
        shape, non-zero = observed pixel): the patches go through the masked ``reconstruct()`` -- inpainting.
        ``weight`` (the image's shape, finite and >= 0): pixel (i, j) was observed with noise variance sigma^2 /
        weight[i, j], 0 = not observed; the patches go through the weighted ``reconstruct()`` (BSC, MCA, MMCA).
        ``aggregate='precision'`` (default ``'mean'``): the overlapping estimates of a pixel are weighted by 1 /
        (V + floor), V each patch's posterior variance there; ``floor`` (default: ``utils.patches.PRECISION_FLOOR`` times the
        mean component variance of MoG; MoP has no noise parameter and needs ``floor=``) and ``window`` (a fixed positive
        weight per patch element, under either aggregate); ``var_map`` is then the average of V under the same weights."""
        from ...utils.patches import denoise_image
        return denoise_image(self, model_params, image, mask=mask, weight=weight, **kw)

    def encode_image(self, model_params, image, mask=None, weight=None, **kw):
        """Feature maps of a whole image: ``utils.patches.encode_image(self, model_params, image, **kw)`` --
        every patch through ``encode()``; returns ``(mean, prob)``, both the responsibilities, as H channels on the patch
        grid, (B, nr, nc, H) or (nr, nc, H) for a 2-D image.  Keywords: ``patch``, ``stride``, ``center``, ``chunk``,
        ``device``, ``exact`` (passed on; the responsibilities are exact already), ``pool`` ((gh, gw) or an int: both results
        pooled over a gh x gw grid of regions of the patch grid into (B, gh, gw, H), a fixed-length feature vector per image)
        and ``reduce`` (``'mean'``, ``'sum'`` or ``'max'``).  ``mask`` and ``weight`` (the image's shape)
        reach ``encode()``, which refuses them for the mixture models by name before any launch.  The bits do not depend on
        ``chunk``."""
        from ...utils.patches import encode_image
        return encode_image(self, model_params, image, mask=mask, weight=weight, **kw)

    def sample_posterior(self, model_params, my_data, n_samples=1, seed=None, latents=False, device=False, uniforms=None,
                         normals=None):
        """Posterior draws of the noiseless data: ``Ys`` (n_samples, my_N, D) float64, Ys[m, n] = W_h with h ~
        r_nh, the responsibilities ``reconstruct`` averages with (the proper densities of ``log_likelihood``); the
        components' own noise is not added.  ``latents=True`` returns ``(Ys, S)``, S (n_samples, my_N, H) one-hot.  NumPy
        arrays, or ``DeviceArray`` handles with ``device=True``; no collective; ``model_params`` and the training shard are
        left as they were.

        U = torch.rand((my_N, n_samples)) from a ``torch.Generator`` on the device seeded with ``seed``, or the caller's
        ``uniforms`` of that shape (NumPy, torch or DeviceArray): then a row's draws depend on that row, the parameters and
        that row of U alone -- the same bits under a row permutation that permutes U along, in a shard and for every
        internal chunking.  With ``seed`` alone the draws depend on (my_N, n_samples): the generator fills the whole array.
        ``normals`` is accepted for the component-analysis models' signature and ignored.  Draw m of row n is the smallest h
        with u C < c_h, c the running sum of the responsibilities in pm_sample_states_f64's order: a component of weight 0 is
        never drawn; a NaN data row gives NaN draws and touches no other row.

        Raises ``ValueError`` for n_samples < 1, a wrongly shaped ``uniforms`` and host ``uniforms`` outside [0, 1),
        ``NotImplementedError`` for ``my_data['mask']`` -- before any launch."""
        return self._sample_posterior(model_params, my_data, n_samples, seed, latents, device, uniforms, normals)

    @tracing.traced
    def generate_data(self, model_params, my_N):
        """Component labels from ``scipy.stats.rv_discrete(values=(arange(H), pies)).rvs(size=my_N)`` (the reference's
        stream, __init__.py:85-98), then ``generate_from_hidden``."""
        H = self.H
        s = stats.rv_discrete(values=(np.arange(H), model_params['pies']), name='compProbDistr').rvs(size=my_N)
        return self.generate_from_hidden(model_params, {'s': s})

    @tracing.traced
    def select_partial_data(self, anneal, data):
        """A random subset of fraction ``anneal['partial']`` of the datapoints (0 or 1: all of them).

        The reference (__init__.py:100-124) calls ``.shape`` on the data dict and cannot run; this does what it sets out
        to do: ``sel = np.random.permutation(my_N)[:my_pN]`` (unsorted, as there) and every per-row entry of the dict
        restricted to ``sel``."""
        partial = anneal['partial']
        if partial == 0 or partial == 1:
            return data
        my_N = data['y'].shape[0]
        my_pN = int(np.ceil(my_N * partial))
        if my_N == my_pN:
            return data
        sel = np.random.permutation(my_N)[:my_pN]
        out = {}
        for key, val in data.items():
            out[key] = val[sel] if getattr(val, 'shape', None) and val.shape[0] == my_N else val
        return out

    @tracing.traced
    def step(self, anneal, model_params, data):
        """noisify -> check -> partial data -> E_step -> M_step, logging as __init__.py:126-149."""
        if self.exact:
            return self.exact_step(anneal, model_params, data)
        self._refuse_training_mask(data)
        model_params = self.noisify_params(model_params, anneal)
        model_params = self.check_params(model_params)
        pdata = self.select_partial_data(anneal, data)
        post_comp_distr = self.E_step(anneal, model_params, pdata)
        new_model_params = self.M_step(anneal, model_params, post_comp_distr, pdata)
        dlog.append_all(new_model_params)
        dlog.append_all(anneal.as_dict())
        return new_model_params

    @tracing.traced
    def inference(self, anneal, model_params, my_data, no_maps=10):
        """Not implemented, as in the reference (__init__.py:151-153)."""
        raise NotImplementedError("MixtureModel.inference is not implemented (nor is it in the reference)")
