"""EM driver and model base class -- the drop-in boundary above the HIP kernels.

Restates prosper/em/__init__.py: ``Model`` (:24-110, incl. ``noisify_params`` :63-107 and
``gain`` :109-110) and ``EM`` (:115-178).  ``EM.run`` is the only entry point that
matters for the hot path: ``while not anneal.finished: model.step(...)``.
"""
import numpy as np

from ..utils import parallel
from ..utils import tracing
from ..utils.datalog import dlog


class Model(object):
    """Abstract EM model: data generation, E/M step, initialisation."""

    def __init__(self, comm=parallel.COMM_WORLD):
        self.comm = comm
        self.noise_policy = {}

    def generate_data(self, model_params, N):
        raise NotImplementedError

    def step(self, anneal, model_params, my_data):
        raise NotImplementedError

    def standard_init(self, data):
        raise NotImplementedError

    # True: ``step`` is one EM step with the posterior over the WHOLE state space, built for BSC_ET; a plain
    # attribute like ``deterministic``.  A model that has no exact step refuses in ``step`` instead of running truncated.
    exact = False

    def exact_step(self, anneal, model_params, my_data):
        """One EM step with the posterior over every latent state: BSC_ET has it."""
        raise NotImplementedError("%s has no exact EM step (exact_step / model.exact = True): BSC_ET has it"
                                  % type(self).__name__)

    def _refuse_training_mask(self, my_data):
        """Training on incomplete data is built for BSC_ET alone: a ``'mask'`` entry is never ignored
        silently -- every other model's ``step`` / ``E_step`` / ``M_step`` refuses it here, before any launch."""
        self._refuse_training_weight(my_data)
        if isinstance(my_data, dict) and my_data.get('mask') is not None:
            raise NotImplementedError("%s: training on incomplete data (my_data['mask'] in step / E_step / M_step) is not "
                                      "built for this model; BSC_ET has the masked EM step" % type(self).__name__)

    def _refuse_training_weight(self, my_data):
        """Per-entry noise weights reach inference only -- ``log_likelihood``, ``reconstruct``,
        ``sample_posterior`` of BSC_ET, MCA_ET and MMCA_ET: a ``'weight'`` entry is never ignored silently -- every model's
        ``step`` / ``select_Hprimes`` / ``E_step`` / ``M_step`` refuses it here, before any launch."""
        if isinstance(my_data, dict) and my_data.get('weight') is not None:
            raise NotImplementedError("%s: training with per-entry noise weights (my_data['weight'] in step / select_Hprimes / "
                                      "E_step / M_step) is not built for any model; log_likelihood, reconstruct and "
                                      "sample_posterior of BSC_ET, MCA_ET and MMCA_ET take a weight" % type(self).__name__)

    @tracing.traced
    def noisify_params(self, model_params, anneal):
        """Add annealed Gaussian noise to parameters named in ``self.noise_policy``
        (value = ``(low, high, absify)``), drawn on rank 0 and broadcast.

        Follows prosper/em/__init__.py:63-107 including its quirk that a *scalar*
        parameter is never actually clipped (the reference assigns the clipped value to
        an unused name, :85-88); array parameters are clipped to [low, high].
        """
        comm = self.comm
        normal = np.random.normal
        for param, (low, high, absify) in self.noise_policy.items():
            pvalue = model_params[param]
            scale = anneal[param + "_noise"]
            if scale != 0.0:
                if np.isscalar(pvalue):
                    new_pvalue = 0
                    if comm.rank == 0:
                        new_pvalue = pvalue + normal(scale=scale)
                        if absify:
                            new_pvalue = np.abs(new_pvalue)
                    pvalue = comm.bcast(new_pvalue)
                else:
                    if comm.rank == 0:
                        noisy = pvalue + normal(scale=scale, size=pvalue.shape)
                        noisy = np.minimum(high, np.maximum(low, noisy))
                        if absify:
                            noisy = np.abs(noisy)
                        pvalue = noisy
                    comm.Bcast([pvalue, parallel.DOUBLE])
            model_params[param] = pvalue
        return model_params

    def gain(self, old_params, new_params):
        return 0.


class EM(object):
    """Drives the annealed EM loop over ``model.step``."""

    def __init__(self, model=None, anneal=None, data=None, lparams=None, mpi_comm=None):
        self.model = model
        self.anneal = anneal
        self.data = data
        self.lparams = lparams
        self.mpi_comm = mpi_comm

    def step(self):
        """One EM step on the current parameters (result discarded, as upstream :138-149)."""
        self.model.step(self.anneal, self.lparams, self.data)

    def run(self, verbose=False):
        """Run a full cooling cycle (prosper/em/__init__.py:152-178)."""
        model, anneal, my_data = self.model, self.anneal, self.data
        model_params = self.lparams
        while not anneal.finished:
            if verbose:
                dlog.progress("EM step %d of %d" % (anneal['step'] + 1, anneal['max_step']),
                              anneal['position'])
            new_model_params = model.step(anneal, model_params, my_data)
            gain = model.gain(model_params, new_model_params)
            anneal.next(gain)
            if anneal.accept:
                model_params = new_model_params
            self.lparams = model_params
