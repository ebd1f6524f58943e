"""Mixture of Poissons: restates prosper/em/mixturemodels/MoP.py with E_step / M_step on the MI355X.

Layouts as there: W (D, H), pies (H,).  ``A`` (not NaN): every datapoint is normalised to total mass A first
(``normalize``), in the E-step and in the M-step alike.
"""
import numpy as np

from . import MixtureModel
from ._device import DeviceMixture, KIND_MOP
from ...utils import parallel
from ...utils import tracing


class MoP(DeviceMixture, MixtureModel):

    def __init__(self, D, H, to_learn=['pies', 'W'], A=np.nan, comm=parallel.COMM_WORLD, device=None):
        """``A <= D`` becomes ``10 * D`` (MoP.py:20-26)."""
        MixtureModel.__init__(self, D=D, H=H, to_learn=to_learn, comm=comm)
        if not np.isnan(A) and A <= D:
            A = 10 * D
        self.A = A
        self._dev_init(device)

    @tracing.traced
    def standard_init(self, my_data):
        """MixtureModel.standard_init, broadcast (MoP.py:29-40).  W may come out negative: its log is then NaN in the
        E-step, as in the reference."""
        model_params = MixtureModel.standard_init(self, my_data)
        return self.comm.bcast(model_params)

    def _seed_rates(self, W):
        """``kmeanspp_init``: a datapoint with a zero count is not a rate (log 0 in the E-step, 0 * -inf = NaN against a zero
        count): W = max(W, eps), the floor the M-step's "+ eps" keeps every rate above (MoP.py:130-160).  Positive counts keep
        their bits."""
        return np.maximum(W, np.finfo(np.float64).eps)

    @tracing.traced
    def resume_init(self, h5_output):
        """W and pies of the last logged step of a ``result.h5`` (MoP.py:42-63, which calls the undefined ``openFile``;
        read here through ``utils.datalog.resume_params``)."""
        from ...utils.datalog import resume_params
        last = resume_params(h5_output, ('W', 'pies'))
        model_params = {}
        if 'W' in self.to_learn:
            model_params['W'] = np.asarray(last['W'])
        if 'pies' in self.to_learn:
            model_params['pies'] = np.asarray(last['pies'])
        return self.comm.bcast(model_params)

    def generate_from_hidden(self, model_params, my_hdata):
        """y[n, d] = Poisson(W[d, s_n]) (MoP.py:65-91).  The reference's per-entry ``np.random.poisson(w, 1)`` calls are one
        ``np.random.poisson`` over the (N, D) rates here: the legacy stream draws them in the same order."""
        s = my_hdata['s']
        W = np.asarray(model_params['W'])
        y = np.random.poisson(W.T[s]).astype(np.float64)
        return {'y': y, 's': s}

    def check_params(self, model_params):
        assert np.isfinite(model_params['W']).all()
        assert np.isfinite(model_params['pies']).all()
        return model_params

    @tracing.traced
    def normalize(self, my_y):
        """((A - D) / (sum_d y + eps)) y + 1 (MoP.py:236-245)."""
        eps = np.finfo(np.float64).eps
        my_y_sum = np.sum(my_y, 1) + eps
        return ((self.A - self.D) / my_y_sum[:, None]) * my_y + 1

    def _rowscale_host(self, y):
        """The row scale of ``normalize``, s_n = (A - D) / (sum_d y + eps): the kernels use s_n y + 1 without storing it."""
        if np.isnan(self.A):
            return None
        eps = np.finfo(np.float64).eps
        return (self.A - self.D) / (np.sum(y, 1) + eps)

    @tracing.traced
    def E_step(self, anneal, model_params, my_data):
        """``posterior`` of the normalised data at beta = 1/T (MoP.py:93-103).  The normalisation ``s y + 1`` is not
        materialised: the kernel scales the rows of the resident raw data by s (``_rowscale_host``) and adds the "+1"
        through the column constant."""
        self._refuse_training_mask(my_data)
        return self._posterior(model_params, my_data['y'], 1. / anneal['T'], raw=True)

    @tracing.traced
    def posterior(self, model_params, my_y, beta=1.0):
        """logpj = beta sum_d (y log w - w) + beta log pies, or with A set beta sum_d y log w (the -w term dropped),
        and posteriors as MoG's (no max subtraction, NaN / tiny / inf clamps) -- MoP.py:176-190 and :193-232.  As in the
        reference ``my_y`` is the data as the model sees it: already normalised (``normalize``) when A is set."""
        return self._posterior(model_params, my_y, beta, raw=False)

    def _posterior(self, model_params, my_y, beta, raw):
        """raw: ``my_y`` is raw data and, with A set, normalised on the fly; else it is taken as it is."""
        W = np.asarray(model_params['W'], dtype=np.float64)
        with np.errstate(all='ignore'):
            lp = np.log(model_params['pies']) * beta
            logW = np.log(W.T)
            if np.isnan(self.A):
                c = -np.sum(W, 0)
            elif not raw:
                c = np.zeros(self.H)          # already normalised data: sum_d y log w as it stands
            else:
                # sum_d (s y + 1) log w = s (y . log w) + sum_d log w: a zero rate's -inf is carried by the second term
                # alone (s y + 1 >= 1 multiplies it in the reference, so -inf for every datapoint; in the first term a
                # zero count would turn it into 0 * -inf = NaN)
                c = np.sum(logW, 1)
                logW = np.where(np.isneginf(logW), 0.0, logW)
        return self._estep_dev(my_y, beta, c, lp, Bl=logW, scaled=raw)

    def _proper_terms(self, model_params):
        """The arguments of the scores kernel for the Poisson pmf on the data the E-step sees: coef = 1, Bl = log W^T on the
        scaled rows, c_h = sum_d log w_dh (the "+1" of x, A set) - sum_d w_dh, lp = log pies."""
        W = np.asarray(model_params['W'], dtype=np.float64)
        normed = not np.isnan(self.A)
        with np.errstate(all='ignore'):
            lp = np.log(np.asarray(model_params['pies'], dtype=np.float64))
            logW = np.log(W.T)
            c = -np.sum(W, 0)
            if normed:
                c = c + np.sum(logW, 1)
                logW = np.where(np.isneginf(logW), 0.0, logW)
            else:
                # a zero rate: pmf 1 at a zero count, 0 otherwise -- y log w with log w = -1e300 gives exactly that weight
                # (0 * -inf would be NaN)
                logW = np.where(np.isneginf(logW), -1e300, logW)
        return {"coef": 1.0, "c": c, "lp": lp, "Bl": logW, "Bq": None, "pmf": 1, "yoff": 1.0 if normed else 0.0}

    def _loglik_rows(self, model_params, res, rows):
        """log_likelihood: rows[n] = log sum_h pies_h prod_d Poisson(x_nd; w_dh) with x = y (A nan) or x = s y + 1 (A set,
        the data the E-step sees): the scores kernel's log-likelihood mode with coef = 1, Bl = log W^T on the scaled rows,
        c_h = sum_d log w_dh (the "+1" of x, A set) - sum_d w_dh, lp = log pies, and the row term - sum_d lgamma(x_nd + 1)."""
        t = self._proper_terms(model_params)
        self._loglik_scores(res, rows, t["coef"], t["c"], t["lp"], t["Bl"], pmf=t["pmf"], yoff=t["yoff"])

    def _recon_scores(self, model_params, res):
        """reconstruct: the log-joints log pies_h + log Poisson(x_n; w_h) up to the row term
        - sum_d lgamma(x_nd + 1), which the responsibilities do not see."""
        return self._proper_logpj(res, self._proper_terms(model_params), scaled=True), 1.0, None

    def log_p_y(self, model_params, my_y, beta=1.0):
        """log_p_y of the reference (MoP.py:193-232): the scores part of ``posterior`` (with pies = 1), an ndarray;
        ``my_y`` as for ``posterior`` (normalised when A is set)."""
        mp = dict(model_params, pies=np.ones(self.H))
        return np.asarray(self.posterior(mp, my_y, beta)['logpj'])

    @tracing.traced
    def M_step(self, anneal, model_params, suff_stats, my_data):
        """MoP.py:105-166 from one packed all-reduce of the device statistics: W_num = Y'^T P for the (normalised) data
        Y' = s Y + 1, i.e. s-scaled Y^T P + colsum(P); W = W_num / sum P + eps, or with A set
        W_num / (colsum(W_num) / A + eps) + eps; pies = (sum P + tiny) normalised.  The given dict is updated and
        returned, as in the reference."""
        self._refuse_training_mask(my_data)
        H, D, A = self.H, self.D, self.A
        tiny = np.finfo(np.float64).tiny
        eps = np.finfo(np.float64).eps
        st = self._mstats(my_data['y'], suff_stats['posteriors_h'], KIND_MOP)
        colsum = st[:H]
        if 'W' in self.to_learn:
            W_num = st[H:H + D * H].reshape(D, H)
            if np.isnan(A):
                sum_posteriors = colsum
            else:
                W_num = W_num + colsum[None, :]
                sum_posteriors = np.sum(W_num, 0) / A + eps
            model_params['W'] = (W_num / sum_posteriors[None, :]) + eps
        if 'pies' in self.to_learn:
            sum_posteriors = colsum + tiny
            model_params['pies'] = sum_posteriors / np.sum(sum_posteriors)
        return model_params
