"""Ternary Sparse Coding on the MI355X: the model of prosper/em/camodels/tsc_et.py.

Latents in {-1, 0, +1} with prior pi/2, 1-pi, pi/2 (scalar ``pi``), linear superposition, Gaussian noise.
Every truncated state lives in the H' candidate positions: the state table holds the null state and the
one-cause states too, ``logpj`` has one column per table row.  Upstream's class cannot be constructed
(``states`` is undefined in tsc_et.py:131); this one can, with the same constructor signature,
``select_Hprimes / E_step / M_step`` signatures, return keys and ``dlog`` side effects (``L``, ``N_use``), and it
reproduces what upstream's methods compute (checked against goldens minted by running them on an object
built without ``__init__``), including two behaviours a caller can observe:

  * candidates are the latents of the H' best one-cause STATES, so a latent can appear twice (tsc_et.py:208-211);
  * for a repeated candidate only its LAST position contributes to the W update (NumPy fancy-index ``+=``,
    tsc_et.py:471-475); pi and sigma see every position.

Kernels: the scores GEMM, ``pm_tsc_select_scores_f64`` + the 16-lane selection kernel over the 2H one-cause
states, and the DSC kernels (csrc/dsc_kernels.hip) with PM_DSC_TABLE_ONLY | PM_DSC_LAST_POSITION.
"""
import itertools as itls

import numpy as np
from scipy.special import comb

from ._device import DeviceArray, _LOG_UNDERFLOW, _ptr
from ._table import TableCAModel
from ... import _lib
from ...utils import parallel
from ...utils import tracing
from ...utils.datalog import dlog

try:
    import torch
except Exception:  # pragma: no cover
    torch = None


def _cut_on_device(c):
    """Data truncation (tsc_et.py:435-446): evidence >= the N_use-th largest ``c``.  The kernel keeps lse > cut; the
    un-stabilised sums upstream cuts on are exactly 0 below the underflow boundary, where `>= 0` keeps every datapoint."""
    ninf = torch.full_like(c, float("-inf"))
    return torch.where(c < _LOG_UNDERFLOW, ninf, torch.nextafter(c, ninf))


def _cut_on_host(c):
    return float("-inf") if c < _LOG_UNDERFLOW else float(np.nextafter(c, -np.inf))


def generate_state_matrix(Hprime, gamma, H, states):
    """(single_state_matrix, state_matrix, no_states, state_abs) as tsc_et.py:23-80 -- incl. ``no_states`` =
    len(states)**Hprime (the size of the untruncated table) and ``state_abs`` over that untruncated table."""
    ss = np.concatenate([np.eye(H, dtype=np.int8) * v for v in states if v != 0])
    single_state_matrix = ss[np.sum(np.abs(ss), 1) == 1]
    s = np.array(list(itls.product(np.array(states), repeat=Hprime)), dtype=np.int8)
    states_abs = np.empty((len(states), s.shape[0]))
    for i in range(len(states)):
        states_abs[i, :] = (s == states[i]).sum(axis=1)
    state_matrix = s[np.sum(np.abs(s), axis=1) <= gamma]
    return single_state_matrix, state_matrix, s.shape[0], states_abs


class TSC_ET(TableCAModel):
    """Ternary Sparse Coding with Expectation Truncation."""

    def __init__(self, D, H, Hprime, gamma, to_learn=['W', 'pi', 'sigma'], comm=parallel.COMM_WORLD, device=None):
        TableCAModel.__init__(self, D, H, Hprime, gamma, to_learn, comm, device)
        self.states = np.array([-1., 0., 1.])
        (self.single_state_matrix, self.state_matrix, self.no_states,
         self.state_abs) = generate_state_matrix(Hprime, gamma, H, self.states)
        tol = 1e-5
        self.noise_policy = {
            'W': (-np.inf, +np.inf, False),
            'pi': (tol, 1. - tol, False),
            'sigma': (0., +np.inf, False),
        }
        self._tab = None

    def _draw_latents(self, model_params, my_N, g):
        pi = float(model_params['pi'])
        p = torch.rand((my_N, self.H), generator=g, device=self.device, dtype=torch.float64)
        one = torch.ones((), dtype=torch.float64, device=self.device)
        return torch.where(p < pi / 2, -one, torch.where(p < pi, one, 0 * one))

    def _generate_data_host(self, model_params, my_N):
        """s_h = -1 / +1 / 0 for p < pi/2, p < pi, else; y = s.W^T + noise.  RNG stream as upstream
        (tsc_et.py:215-275): ``random(H)`` per datapoint, then one ``normal((my_N, D))``."""
        pi = model_params['pi']
        W = model_params['W'].T
        p = np.random.random(size=(my_N, self.H))
        s = np.where(p < pi / 2, -1, np.where(p < pi, 1, 0)).astype(np.int8)
        y = s.astype(np.float64) @ W
        y += np.random.normal(scale=model_params['sigma'], size=(my_N, self.D))
        return {'y': y, 's': s}

    def inference(self, anneal, model_params, test_data, topK=10, logprob=False, abs_marginal=True,
                  adaptive=True, Hprime_max=None, gamma_max=None, exact=False):
        """Top-K posterior states, signed marginal ``m`` and absolute marginal ``am`` per datapoint
        (tsc_et.py:546-680); same return dict.  As upstream: ``p`` is the normalised probability (its log with
        ``logprob``), a repeated candidate's LAST position wins the writes into ``s`` / ``m`` / ``am``, re-run
        datapoints keep earlier entries, and datapoints whose best state has exactly gamma non-zeros are re-run
        with Hprime+1 / gamma+1."""
        if exact:           # (refused by name, before any launch: DeviceCAModel._inference_exact_admit)
            self._inference_exact_admit(anneal, model_params, test_data, topK, Hprime_max, gamma_max)
        assert 'y' in test_data, "Key 'y' in test_data dict not defined."
        H, dev = self.H, self.device
        res_am = torch.zeros((test_data['y'].shape[0], H), dtype=torch.float64, device=dev)

        def run_pass(lp, cd, k_eff, ind_n, buf):
            n_cur, S = lp.shape
            Hp = self.Hprime
            # top-K states, signed / absolute marginals and the writes into s / m / am in position order: one HIP pass
            # (pm_infer_topk_signed_f64).  States that differ only in WHICH position of a repeated candidate is active tie
            # exactly, and the order NumPy's argsort()[::-1] (tsc_et.py:626, an introsort) gives exact ties is not a
            # function of (value, column): the kernel flags the rows with a tie among their topK + 1 best, those -- a
            # handful -- are ranked with NumPy itself, and the pass runs again with the ranking handed in.
            cd32 = cd.to(torch.int32).contiguous()
            vals = torch.from_numpy(np.ascontiguousarray(self.state_matrix.astype(np.int8))).to(dev)
            top_idx = torch.empty((n_cur, k_eff), dtype=torch.int32, device=dev)
            top_lpc = torch.empty((n_cur, k_eff), dtype=torch.float64, device=dev)
            top_post = torch.empty((n_cur, k_eff), dtype=torch.float64, device=dev)
            tie = torch.zeros(n_cur, dtype=torch.int32, device=dev)
            s_blk = buf['s'][ind_n, :k_eff].contiguous()
            m_blk, am_blk = buf['m'][ind_n].contiguous(), res_am[ind_n].contiguous()

            def run(rank):
                self._call("infer_topk", "pm_infer_topk_signed_f64", _ptr(lp), lp.stride(0), _ptr(cd32), _ptr(vals), n_cur,
                           H, Hp, S, k_eff, rank, _ptr(top_idx), _ptr(top_lpc), _ptr(top_post), _ptr(tie), _ptr(s_blk),
                           _ptr(m_blk), _ptr(am_blk) if abs_marginal else None, self._stream())
            run(1)
            self._refuse_nan(top_idx)
            tied = torch.nonzero(tie).flatten()
            if tied.numel():
                rows = lp[tied].cpu().numpy()
                rel = rows - rows.max(axis=1, keepdims=True)
                lpc = rel - np.log(np.exp(rel).sum(axis=1, keepdims=True))
                order = np.argsort(lpc, axis=-1)[:, ::-1][:, :k_eff]
                top_idx[tied] = torch.from_numpy(np.ascontiguousarray(order).astype(np.int32)).to(dev)
                run(0)
            buf['s'][ind_n, :k_eff] = s_blk
            buf['m'][ind_n] = m_blk
            res_am[ind_n] = am_blk
            buf['p'][ind_n, :k_eff] = top_lpc if logprob else top_post

        def regenerate():
            (self.single_state_matrix, self.state_matrix, self.no_states,
             self.state_abs) = generate_state_matrix(self.Hprime, self.gamma, self.H, self.states)

        def restore():
            self.comm.Barrier()
            regenerate()

        buf = self._adaptive_inference(anneal, model_params, test_data, topK, adaptive, Hprime_max, gamma_max,
                                       run_pass, regenerate, restore)
        with np.errstate(divide='ignore'):
            m_out = buf['m'].cpu().numpy()
            am_out = res_am.cpu().numpy()
            if logprob:
                m_out, am_out = np.log(m_out), np.log(am_out)
        return {'s': buf['s'].cpu().numpy(), 'm': m_out, 'am': am_out, 'p': buf['p'].cpu().numpy(),
                'gamma': buf['gamma'].cpu().numpy(), 'Hprime': buf['Hprime'].cpu().numpy()}

    # ------------------------------------------------------------------ plumbing
    def _tables(self):
        key = (self.Hprime, self.gamma, self.state_matrix.shape[0])
        if self._tab is None or self._tab[0] != key:
            if not _lib.load().pm_bsc_rows16_supported(2 * self.H, self.Hprime, 0):
                raise _lib.HipError("TSC_ET: 2 H = %d one-cause states exceed the selection kernel's range (<= 512)"
                                    % (2 * self.H))
            idx = (self.state_matrix.astype(np.int64) + 1).astype(np.uint8)       # -1, 0, +1 -> 0, 1, 2
            self._tab = (key, torch.from_numpy(np.ascontiguousarray(idx)).to(self.device))
        return self._tab[1]

    def _params(self, anneal, pi, sigma):
        beta = 1. / anneal['T']
        pre1 = -1. / 2. / sigma / sigma
        P = _lib.DscParams(K=3, K0=1, pre1=float(pre1), ecoef=float(beta * pre1),
                           pscale=float(beta if anneal['anneal_prior'] else 1.0), flags=1 | 2)
        for k in range(3):
            P.values[k] = float(self.states[k])
        return P

    def _prior(self, pi):
        """log prior of every table row over the H' positions (tsc_et.py:327-337)."""
        pm = np.where(self.state_matrix != 0, pi / 2, 1 - pi)
        return np.log(pm).sum(axis=1)

    def _params_dev(self, W, res):
        """Device copy of W^T (H,D), the Gram matrix and the scores for the current W and data."""
        return self._scores_params(W, res)

    # ------------------------------------------------------------------ hot path
    @tracing.traced
    def select_Hprimes(self, model_params, data):
        """``data['candidates']`` (N, Hprime): latents of the Hprime best one-cause states, best last; a latent
        may repeat (tsc_et.py:142-213)."""
        self._refuse_training_weight(data)
        res = self._resident(data['y'])
        N = res["Y"].shape[0]
        H, Hp = self.H, self.Hprime
        self._tables()
        par = self._params_dev(model_params['W'], res)
        cand = torch.empty((N, Hp), dtype=torch.int32, device=self.device)
        if N and _lib.load().pm_xsc_select_supported(H, Hp, 1):
            # the 2 H one-cause values formed and ranked in one pass over the scores; candidates come out as latents
            self._call("select", "pm_xsc_select_f64", _ptr(par["A"]), H, _ptr(par["G"]), None, N, H, Hp, _ptr(cand),
                       self._stream())
        elif N:
            R = self._buf("tsc_sel", (N, 2 * H))
            self._call("select_scores", "pm_tsc_select_scores_f64", _ptr(par["A"]), H, _ptr(par["G"]), N, H, _ptr(R),
                       2 * H, self._stream())
            # raw mode ranks R itself; the Gram / norm arguments only need to be valid memory
            gdummy = self._buf("tsc_gdummy", (2 * H, 2 * H))
            self._call("select", "pm_bsc_select_estep_f64", _ptr(R), 2 * H, _ptr(gdummy), _ptr(res["ynorm2"]), None, None,
                       None, None, None, 0, self.gamma, None, N, 2 * H, Hp, 1 | 8, _ptr(cand), None, 0, None,
                       self._stream())
            cand = torch.remainder(cand, H)            # state index -> latent index (tsc_et.py:210)
        data['candidates'] = DeviceArray(cand, np.int64)
        return data

    @tracing.traced
    def E_step(self, anneal, model_params, my_data):
        """Log-pseudo-joints ``{'logpj': (N, S)}``, one column per table row (tsc_et.py:277-356)."""
        self._refuse_training_mask(my_data)
        res = self._resident(my_data['y'])
        N = res["Y"].shape[0]
        S = self.state_matrix.shape[0]
        tab = self._tables()
        par = self._params_dev(model_params['W'], res)
        cand = self._device_candidates(my_data['candidates'], N)
        P = self._params(anneal, model_params['pi'], model_params['sigma'])
        prior = self._upload(self._prior_ws, self._prior(model_params['pi']))
        tracing.tracepoint("E_step:iterating")
        return {'logpj': self._dsc_estep(anneal, self._stats_ws, par, res, cand, tab, S, prior, P, S, [model_params['pi']])}

    def _loglik_terms(self, model_params, my_data):
        """log_likelihood.  At T = 1 a column of ``logpj`` is - |y - W s|^2 / (2 sigma^2) plus the log-prior of
        the state's Hprime candidate positions only (pi / 2 for -1 and +1, 1 - pi for 0; tsc_et.py:320-351): the H - Hprime
        other latents are 0 with probability 1 - pi each, so c = (H - Hprime) log(1 - pi) - D/2 log(2 pi sigma^2) -- the
        reference's ``L`` (tsc_et.py:447-451) without its - log A_pi_gamma, plus the missing prior -- and a = 1."""
        pies, sigma = float(model_params['pi']), float(model_params['sigma'])
        c = (self.H - self.Hprime) * np.log(1. - pies) - 0.5 * self.D * np.log(2 * np.pi * sigma ** 2)
        return self._loglik_estep(model_params, my_data), 1.0, c

    def _recon_layout(self, model_params):
        """reconstruct: one column per row of the ternary state table (values -1 / 0 / +1 per candidate
        POSITION), no null / one-cause prefix; ybar(s) = sum_j s_j W_{cand_j}: a latent that two positions hold is counted at
        both, as in the E-step's energy."""
        return {"params": model_params, "blocks": (), "soff": 0, "moff": 0, "table": self.state_matrix,
                "W": model_params['W'], "mu": None}

    def _loglik_exact(self, model_params):
        """exact log_likelihood: states {-1,0,1}^H, log prior nz(s) log(pi / 2) + (H - nz(s)) log(1 - pi)."""
        pi = float(model_params['pi'])
        with np.errstate(divide='ignore'):
            lp = np.log([0.5 * pi, 1. - pi, 0.5 * pi])
        return self._exact_linear(model_params['W'], model_params['sigma'], [-1., 0., 1.], np.tile(lp, (self.H, 1)))

    # ------------------------------------------------------------------ what TableCAModel.M_step asks of the model
    _stats_ws, _prior_ws = "tsc_stats", "tsc_prior"
    _cut_rule = (_cut_on_device, _cut_on_host)

    def _n_logpj(self):
        return self.state_matrix.shape[0]

    def _prior_factors(self, model_params):
        """Factors of the pi update (tsc_et.py:425-432)."""
        H, gamma, pi = self.H, self.gamma, model_params['pi']
        A_pi_gamma = 0.0
        B_pi_gamma = 0.0
        for gam1 in range(gamma + 1):
            for gam2 in range(gamma - gam1 + 1):
                cmb = comb(gam1, gam1) * comb(gam1 + gam2, gam2) * comb(H, H - gam1 - gam2)
                t = cmb * ((pi / 2) ** (gam1 + gam2)) * ((1 - pi) ** (H - gam1 - gam2))
                A_pi_gamma += t
                B_pi_gamma += (gam1 + gam2) * t
        E_pi_gamma = pi * H * A_pi_gamma / B_pi_gamma
        return pi, [pi], A_pi_gamma, (A_pi_gamma, E_pi_gamma)

    def _finalize(self, stats, model_params, A_pi_gamma, E_pi_gamma):
        """Parameter updates from the all-reduced statistics (tsc_et.py:448-542), one device->host copy.  Logs ``L`` and
        ``N_use``.  A singular Wq goes to the reference's pseudo-inverse (tsc_et.py:488)."""
        H, D = self.H, self.D
        pi, sigma = model_params['pi'], model_params['sigma']
        host, W_out = self._update_W(stats, model_params, lambda Wq, Wp: np.dot(np.linalg.pinv(Wq), Wp))
        cnt = host[:8]
        my_sigma, Fs, N_use = float(host[8]), float(host[9]), int(round(host[10]))

        L = -0.5 * D * np.log(2 * np.pi * sigma ** 2) - np.log(A_pi_gamma) + Fs / N_use      # tsc_et.py:449-453
        dlog.append('L', L)

        if 'pi' in self.to_learn:
            tracing.tracepoint("M_step:update pi")
            pi_new = E_pi_gamma * (cnt[0] + cnt[2]) / H / N_use          # expected number of non-zero latents
        else:
            pi_new = pi
        if 'sigma' in self.to_learn:
            tracing.tracepoint("M_step:update sigma")
            sigma_new = np.sqrt(my_sigma / D / N_use)
        else:
            sigma_new = sigma
        dlog.append('N_use', N_use)
        return {'W': W_out, 'pi': pi_new, 'sigma': sigma_new, 'Q': 0.}
