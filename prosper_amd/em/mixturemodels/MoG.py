"""Mixture of Gaussians: restates prosper/em/mixturemodels/MoG.py with E_step / M_step on the MI355X.

Layouts as there: W (D, H), pies (H,), sigmas_sq (H, D) for ``sigmas_sq_type='diagonal'`` and (H, D, D) for 'full'.
"""
import numpy as np

from . import MixtureModel, _host
from ._device import DeviceMixture, KIND_DIAG, KIND_FULL
from ...utils import parallel
from ...utils import tracing


class MoG(DeviceMixture, MixtureModel):

    def __init__(self, D, H, to_learn=['pies', 'W', 'sigmas_sq'], sigmas_sq_type='full', comm=parallel.COMM_WORLD,
                 device=None):
        MixtureModel.__init__(self, D=D, H=H, to_learn=to_learn, comm=comm)
        self.sigmas_sq_type = sigmas_sq_type
        self._dev_init(device)

    @tracing.traced
    def standard_init(self, my_data):
        """MixtureModel.standard_init, then every component's covariance = rank 0's LOCAL data covariance, broadcast
        (MoG.py:23-60): ``np.cov(y.T) + 0.001 I`` (ddof 1) for 'full', ``np.var(y, 0) + 0.001`` (ddof 0) for 'diagonal'.
        The collective min / max of the data the reference computes there (unused) are computed as well."""
        my_y = _host(my_data['y'])
        model_params = MixtureModel.standard_init(self, {'y': my_y})
        return self.comm.bcast(self._init_noise(model_params, {'y': my_y}))

    def _init_noise(self, model_params, my_data):
        """sigmas_sq of ``standard_init`` (MoG.py:41-58), for ``kmeanspp_init`` too."""
        comm = self.comm
        H = self.H
        my_y = _host(my_data['y'])
        N, D = my_y.shape
        if 'sigmas_sq' in self.to_learn:
            if self.sigmas_sq_type == 'full':
                sigma = comm.bcast(np.cov(my_y.T) + (0.001 * np.eye(D)))
            elif self.sigmas_sq_type == 'diagonal':
                sigma = comm.bcast(np.var(my_y, axis=0) + 0.001)
            np.min(comm.allgather(np.min(my_y, 0)))
            np.max(comm.allgather(np.max(my_y, 0)))
            sigmas_sq = np.zeros(tuple([H]) + sigma.shape)
            for h in range(H):
                sigmas_sq[h] = sigma
            model_params['sigmas_sq'] = sigmas_sq
        return model_params

    @tracing.traced
    def resume_init(self, h5_output):
        """Parameters of the last logged step of a ``result.h5`` (MoG.py:62-100, which calls the undefined ``openFile``
        and cannot run; read here through ``utils.datalog.resume_params``).  sigmas_sq stored in the other layout is
        converted: full -> its diagonals, diagonal -> diagonal matrices."""
        from ...utils.datalog import resume_params
        last = resume_params(h5_output, ('W', 'pies', 'sigmas_sq'))
        model_params = {}
        if 'W' in self.to_learn:
            model_params['W'] = np.asarray(last['W'])
        if 'pies' in self.to_learn:
            model_params['pies'] = np.asarray(last['pies'])
        if 'sigmas_sq' in self.to_learn:
            prev = np.asarray(last['sigmas_sq'])
            sigmas_sq = prev.copy()
            if prev.ndim == 3 and self.sigmas_sq_type == 'diagonal':
                sigmas_sq = np.array([prev[h].diagonal() for h in range(prev.shape[0])])
            elif prev.ndim == 2 and self.sigmas_sq_type == 'full':
                sigmas_sq = np.array([np.diag(prev[h]) for h in range(prev.shape[0])])
            model_params['sigmas_sq'] = sigmas_sq
        return self.comm.bcast(model_params)

    def generate_from_hidden(self, model_params, my_hdata):
        """y_n = w_{s_n} + sqrt(diag sigma_{s_n}) * randn(D) (MoG.py:102-131: also for 'full' only the diagonal enters).
        The per-datapoint ``np.random.randn(D)`` calls are one ``randn(N, D)`` here: the legacy stream is the same."""
        D = self.D
        s = my_hdata['s']
        my_N = s.size
        W = model_params['W'].T
        if self.sigmas_sq_type == 'full':
            sig = np.array([model_params['sigmas_sq'][h].diagonal() for h in range(self.H)])
        else:
            sig = np.asarray(model_params['sigmas_sq'])
        y = W[s] + np.sqrt(sig[s]) * np.random.randn(my_N, D).reshape(my_N, D)
        return {'y': y, 's': s}

    def _noise_variance(self, model_params):
        """The mean variance over components and dimensions (of a full covariance: its diagonal): what
        ``reconstruct_image(aggregate='precision')`` scales its default floor by."""
        sig = np.asarray(model_params['sigmas_sq'], dtype=np.float64)
        return float(np.mean(np.diagonal(sig, axis1=1, axis2=2)) if sig.ndim == 3 else np.mean(sig))

    def check_params(self, model_params):
        assert np.isfinite(model_params['W']).all()
        assert np.isfinite(model_params['sigmas_sq']).all()
        assert np.isfinite(model_params['pies']).all()
        return model_params

    @tracing.traced
    def E_step(self, anneal, model_params, my_data):
        """``posterior(model_params, y, 1/T)`` (MoG.py:133-140)."""
        self._refuse_training_mask(my_data)
        return self.posterior(model_params, my_data['y'], 1. / anneal['T'])

    @tracing.traced
    def posterior(self, model_params, my_y, beta=1.0):
        """logpj = -(logdet_h + maha)·beta + beta·log(pies) with NO factor 1/2 (MoG.py:213-281), and posteriors
        exp(logpj) with no max subtraction: NaN -> tiny, < tiny -> tiny, inf -> max/H, then normalised per row.

        diagonal: logdet = sum log sigma^2; the scores kernel forms maha in expanded form,
            [y^2, y] . [1/sigma^2 ; -2 w/sigma^2] + sum w^2/sigma^2,
          and a component with any sigma^2 <= 0 is NaN throughout, as in the reference (log of a negative, or
          -inf + inf for a zero).
        full: a batched Cholesky on the device gives L^-1 and log det for every positive definite covariance, and
          maha = |L^-1 (y - w)|^2; a component it rejects (indefinite, singular) falls back to the reference's own
          ``np.linalg.inv`` + ``slogdet(sigma)[1]`` (log |det|, sign dropped) on the host, for that component only, and
          maha = (y - w) Sigma^-1 (y - w)^T.  ``fallback_components`` lists those of the last E-step."""
        H = self.H
        W = np.asarray(model_params['W'], dtype=np.float64)
        sig = np.asarray(model_params['sigmas_sq'], dtype=np.float64)
        with np.errstate(all='ignore'):
            lp = np.log(model_params['pies']) * beta
            if self.sigmas_sq_type == 'full':
                B, mode, logdet = self._full_factors(sig)
                return self._estep_dev(my_y, -beta, logdet, lp, W_rows=W.T, B=B, mode=mode)
            Bq = 1. / sig
            Bl = -2. * W.T * Bq
            c = np.sum(W.T ** 2 * Bq, 1) + np.sum(np.log(sig), 1)
            c[(sig <= 0).any(1)] = np.nan
        return self._estep_dev(my_y, -beta, c, lp, Bl=Bl, Bq=Bq)

    def _proper_terms(self, model_params):
        """The arguments of the scores kernel for the proper diagonal density: (S[n,h] + c_h) coef + lp_h = log pies_h +
        log N(y_n; w_h, diag sigma_h^2), coef = -1/2, c_h = sum_d w^2/sigma^2 + sum_d log sigma^2, lp_h = log pies_h -
        D/2 log(2 pi)."""
        W = np.asarray(model_params['W'], dtype=np.float64)
        sig = np.asarray(model_params['sigmas_sq'], dtype=np.float64)
        pies = np.asarray(model_params['pies'], dtype=np.float64)
        with np.errstate(all='ignore'):
            lp = np.log(pies) - 0.5 * self.D * np.log(2 * np.pi)
            Bq = 1. / sig
            Bl = -2. * W.T * Bq
            c = np.sum(W.T ** 2 * Bq, 1) + np.sum(np.log(sig), 1)
            c[(sig <= 0).any(1)] = np.nan
        return {"coef": -0.5, "c": c, "lp": lp, "Bl": Bl, "Bq": Bq}

    def _loglik_rows(self, model_params, res, rows):
        """log_likelihood: rows[n] = log sum_h pies_h N(y_n; w_h, Sigma_h).  Diagonal: the scores kernel's log-likelihood
        mode with coef = -1/2, c_h = sum_d w^2/sigma^2 + sum_d log sigma^2 and lp_h = log pies_h - D/2 log(2 pi).  Full:
        ``_loglik_full``."""
        if self.sigmas_sq_type == 'full':
            return self._loglik_full(res, rows, np.asarray(model_params['W'], dtype=np.float64),
                                     np.asarray(model_params['sigmas_sq'], dtype=np.float64),
                                     np.asarray(model_params['pies'], dtype=np.float64))
        t = self._proper_terms(model_params)
        self._loglik_scores(res, rows, t["coef"], t["c"], t["lp"], t["Bl"], Bq=t["Bq"])

    def _recon_scores(self, model_params, res):
        """reconstruct: ``(X, a, offsets)`` with r_nh = softmax_h(a X[n,h] + o_h) the responsibilities of the
        proper densities -- diagonal: the scores kernel's log-joints; full: the Mahalanobis terms of ``_loglik_full``."""
        if self.sigmas_sq_type == 'full':
            M, off_d = self._full_scores(res, np.asarray(model_params['W'], dtype=np.float64),
                                         np.asarray(model_params['sigmas_sq'], dtype=np.float64),
                                         np.asarray(model_params['pies'], dtype=np.float64))
            return M, -0.5, off_d
        return self._proper_logpj(res, self._proper_terms(model_params)), 1.0, None

    def log_p_y(self, model_params, my_y, beta=1.0):
        """log_p_y of the reference (MoG.py:231-281): the scores part of ``posterior`` (with pies = 1), an ndarray."""
        mp = dict(model_params, pies=np.ones(self.H))
        return np.asarray(self.posterior(mp, my_y, beta)['logpj'])

    @tracing.traced
    def M_step(self, anneal, model_params, suff_stats, my_data):
        """MoG.py:142-202 from one packed all-reduce of the device statistics:
        W = (Y^T P) / (sum P + tiny); diagonal sigma^2 = (Y^2)^T P / sum - W^2; full sigma_h = sum_n p_nh y_n y_n^T / sum_h
        - w_h w_h^T (un-centred, with the new W when W is learned); pies = sum / sum(sum).  As in the reference the
        given parameter dict is updated and returned."""
        self._refuse_training_mask(my_data)
        H, D = self.H, self.D
        tiny = np.finfo(np.float64).tiny
        full = self.sigmas_sq_type == 'full'
        st = self._mstats(my_data['y'], suff_stats['posteriors_h'], KIND_FULL if full else KIND_DIAG)
        sum_posteriors = st[:H] + tiny
        if 'W' in self.to_learn:
            W_num = st[H:H + D * H].reshape(D, H)
            model_params['W'] = W_num * np.power(sum_posteriors, -1)[None, :]
        if 'sigmas_sq' in self.to_learn:
            if full:
                sigmas_sq = st[H + D * H:].reshape(H, D, D)
                model_params['sigmas_sq'] = sigmas_sq * np.power(sum_posteriors, -1)[:, None, None]
                for h in range(H):
                    model_params['sigmas_sq'][h, :, :] -= np.outer(model_params['W'][:, h], model_params['W'][:, h])
            else:
                sigmas_sq = st[H + D * H:].reshape(D, H).T
                model_params['sigmas_sq'] = sigmas_sq * np.power(sum_posteriors, -1)[:, None]
                model_params['sigmas_sq'] -= model_params['W'].T ** 2
        if 'pies' in self.to_learn:
            model_params['pies'] = sum_posteriors / np.sum(sum_posteriors)
        return model_params
