"""Device plumbing of the mixture models: the resident data shard, workspaces, and the calls into the pm_mix_* entries
of libprosper_hip.so (include/prosper_hip.h, csrc/mixture_kernels.hip).  PyTorch supplies memory and streams; every
computation over the datapoints is a HIP kernel, and there is no CPU fallback."""
import ctypes

import numpy as np

from ... import _lib
from ..camodels._device import DeviceArray, _ptr

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

KIND_MOP, KIND_DIAG, KIND_FULL = 0, 1, 2      # the `kind` of pm_mix_mstats_f64


class DeviceMixture(object):
    """Mixin of ``MoG`` / ``MoP``: one MI355X per rank."""

    _device = None

    def _dev_init(self, device=None):
        self._device = device
        self._data = {}
        self._ws = {}

    @property
    def device(self):
        if self._device is None:
            if torch is None or not torch.cuda.is_available():
                raise _lib.HipError("%s needs a HIP device: the hot path has no CPU fallback" % type(self).__name__)
            self._device = torch.device("cuda", torch.cuda.current_device())
        return torch.device(self._device)

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _buf(self, name, shape):
        t = self._ws.get(name)
        if t is None or tuple(t.shape) != tuple(shape):
            t = self._ws[name] = torch.empty(shape, dtype=torch.float64, device=self.device)
        return t

    def _dev(self, host):
        return torch.from_numpy(np.ascontiguousarray(host, dtype=np.float64)).to(self.device)

    def _rowscale_host(self, y):
        """Per-datapoint row scale of the data (None: no scaling).  MoP overrides it."""
        return None

    def _resident(self, y):
        """Device copy of a data shard (+ its row scale), uploaded once per array: recognised by the identity of the
        caller's array and a strided fingerprint (``select_partial_data`` builds a fresh ``y[sel]`` each step)."""
        src = y
        if isinstance(y, DeviceArray):
            y = y.tensor
        d = self._data
        if torch.is_tensor(y):
            ver = (y._version, tuple(y.shape))
        else:
            y = np.asarray(y)
            n = y.shape[0]
            ver = (float(y[::max(1, n // 16)].sum()) if n else 0.0, y.shape)
        if d and d["src"] is src and d["ver"] == ver:
            return d
        if torch.is_tensor(y):
            Y = y.to(device=self.device, dtype=torch.float64).contiguous()
            yh = None
        else:
            yh = np.ascontiguousarray(y, dtype=np.float64)
            Y = torch.from_numpy(yh).to(self.device)
        assert Y.dim() == 2 and Y.shape[1] == self.D
        rs = self._rowscale_host(yh if yh is not None else Y.cpu().numpy())
        self._data = {"src": src, "ver": ver, "Y": Y, "rs": None if rs is None else self._dev(rs)}
        return self._data

    def invalidate_data(self):
        """Forget the resident shards, the training one and the one of ``log_likelihood`` (call after modifying
        ``my_data['y']`` in place, or to release the held-out data's device memory)."""
        self._data = {}
        self.__dict__.pop("_eval_slot", None)

    def _refuse_mask(self, my_data):
        """Missing values are built for BSC and MCA / MMCA only: a mask is refused before any launch, never
        ignored."""
        if my_data.get('mask') is not None:
            raise NotImplementedError("%s: missing values (my_data['mask']) are not built for the mixture models; BSC_ET, "
                                      "MCA_ET and MMCA_ET have the masked E-step" % type(self).__name__)
        if my_data.get('weight') is not None:
            raise NotImplementedError("%s: per-entry noise weights (my_data['weight']) are not built for the mixture models; "
                                      "BSC_ET, MCA_ET and MMCA_ET have the weighted E-step" % type(self).__name__)

    # ---- held-out log-likelihood --------------------------------------------------------------------------
    def log_likelihood(self, model_params, my_data, per_datapoint=False, exact=False):
        """Exact held-out log-likelihood sum_n log sum_h pies_h p(y_n | h) of ``my_data['y']`` (host array, torch tensor or
        DeviceArray) with the proper densities: MoG with the 1/2 and (2 pi)^(-D/2) factors (diagonal: sum_d log sigma^2;
        full: log det from the device Cholesky), MoP the Poisson pmf including - sum_d lgamma(y_nd + 1) on the data the
        E-step sees (normalised when A is set).  The reference's E-step quirk (no 1/2, MoG.py:213-281) stays in E_step /
        posterior / log_p_y; this method does not reuse it.

        Returns the sum over ALL ranks' datapoints as a float (collective; per-rank sums added in rank order, the same bits
        on every rank), or with ``per_datapoint=True`` this rank's (my_N,) float64 values.  A component with pies_h > 0 whose
        full covariance the Cholesky rejects makes every row NaN, a NaN in a data row that row.  ``model_params`` and the
        training shard are left as they were (the evaluation keeps its data and workspaces in a slot of its own).
        ``exact`` is accepted for the component-analysis models' signature: a mixture's value is exact either
        way, and ``exact=True`` returns the same bits.  ``my_data['mask']`` (missing values) is refused."""
        self._refuse_mask(my_data)
        saved = dict(self.__dict__)
        slot = saved.get("_eval_slot") or {"_data": {}, "_ws": {}}
        self._data, self._ws = slot["_data"], slot["_ws"]
        try:
            res = self._resident(my_data['y'])
            N = res["Y"].shape[0]
            lib = _lib.load()
            rows = torch.empty(N, dtype=torch.float64, device=self.device)
            if N:
                self._loglik_rows(dict(model_params), res, rows)
            work = torch.empty(int(lib.pm_rows_lse_work_len(N)), dtype=torch.float64, device=self.device)
            total = torch.empty(1, dtype=torch.float64, device=self.device)
            # (the ordered total of the rows: the log-sum-exp of a row of one entry is that entry)
            _lib.call("pm_rows_lse_f64", _ptr(rows), 1, N, 1, 1.0, None, None, _ptr(work), _ptr(total), self._stream())
            out = rows.cpu().numpy() if per_datapoint else float(total.cpu()[0])
        finally:
            slot = {"_data": self._data, "_ws": self._ws}
            self.__dict__.clear()
            self.__dict__.update(saved)
            self._eval_slot = slot
        if per_datapoint:
            return out
        acc = 0.0
        for v in self.comm.allgather(out):
            acc += v
        return acc

    def _loglik_scores(self, res, rows, coef, c, lp, Bl, Bq=None, pmf=0, yoff=0.0):
        """pm_mix_loglik_f64: rows[n] = log sum_h exp((S[n,h] + c_h) coef + lp_h) - (pmf: sum_d lgamma(s_n y_nd + yoff + 1))."""
        Y, H, D = res["Y"], self.H, self.D
        # (the device copies are held here until the launch: a temporary freed inside the argument list hands its block to
        # the next upload)
        Bq_d = self._dev(Bq) if Bq is not None else None
        Bl_d, c_d, lp_d = self._dev(Bl), self._dev(c), self._dev(lp)
        _lib.call("pm_mix_loglik_f64", _ptr(Y), D, _ptr(res["rs"]) if pmf else None, _ptr(Bq_d), _ptr(Bl_d), D, _ptr(c_d),
                  float(coef), _ptr(lp_d), Y.shape[0], D, H, int(pmf), float(yoff), _ptr(rows), self._stream())

    def _full_scores(self, res, W, sig, pies):
        """MoG full: pm_mix_chol_f64 -> L^-1, log det per component; pm_mix_maha_f64 -> M[n,h] = |L^-1 (y - w)|^2 (N, H) and
        the column offsets log pies_h - 1/2 log det_h - D/2 log(2 pi), so that log pies_h N(y_n; w_h, Sigma_h) = - M / 2 +
        offset.  A component the Cholesky rejects gets a zero B in mode 1 (M = 0) and offset NaN (pies_h > 0) or -inf
        (pies_h = 0).  Returns the device pair (M, offsets)."""
        H, D = self.H, self.D
        Y = res["Y"]
        N = Y.shape[0]
        S_d = self._dev(sig)
        Lw = self._buf("ll_chol_L", (H, D, D))
        B = self._buf("ll_chol_B", (H, D, D))
        logdet_d = torch.empty(H, dtype=torch.float64, device=self.device)
        status_d = torch.empty(H, dtype=torch.int32, device=self.device)
        st = self._stream()
        _lib.call("pm_mix_chol_f64", _ptr(S_d), D, H, _ptr(Lw), _ptr(B), _ptr(logdet_d), _ptr(status_d), st)
        status = status_d.cpu().numpy()
        logdet = logdet_d.cpu().numpy().copy()
        bad = np.nonzero(status)[0]
        mode = np.zeros(H, dtype=np.int32)
        for h in bad:
            B[h].zero_()
            mode[h] = 1
        with np.errstate(divide='ignore', invalid='ignore'):
            off = np.log(pies) - 0.5 * logdet - 0.5 * D * np.log(2 * np.pi)
        off[bad] = np.where(pies[bad] > 0, np.nan, -np.inf)
        mode_d = torch.from_numpy(mode).to(self.device)
        M = self._buf("ll_maha", (N, H))
        W_d, off_d = self._dev(W.T), self._dev(off)
        _lib.call("pm_mix_maha_f64", _ptr(Y), D, _ptr(W_d), _ptr(B), _ptr(mode_d), N, D, H, _ptr(M), H, st)
        return M, off_d

    def _loglik_full(self, res, rows, W, sig, pies):
        """MoG full: ``_full_scores``, then pm_rows_lse_f64 with a = -1/2 and the column offsets."""
        N = res["Y"].shape[0]
        M, off_d = self._full_scores(res, W, sig, pies)
        work = torch.empty(int(_lib.load().pm_rows_lse_work_len(N)), dtype=torch.float64, device=self.device)
        total = torch.empty(1, dtype=torch.float64, device=self.device)
        _lib.call("pm_rows_lse_f64", _ptr(M), self.H, N, self.H, -0.5, _ptr(off_d), _ptr(rows), _ptr(work), _ptr(total),
                  self._stream())

    # ---- posterior-mean reconstruction ------------------------------------------------------------------
    def _proper_logpj(self, res, t, scaled=False):
        """pm_mix_scores_f64 with the proper densities' terms ``t`` (``_proper_terms``): the (N, H) device log-joints
        (S + c_h) coef + lp_h.  (The posteriors the kernel writes beside them are the reference's un-stabilised ones and
        are not used.)"""
        Y, H, D = res["Y"], self.H, self.D
        N = Y.shape[0]
        logpj = self._buf("recon_logpj", (N, H))
        post = self._buf("recon_post", (N, H))
        Bq_d = self._dev(t["Bq"]) if t.get("Bq") is not None else None
        Bl_d, c_d, lp_d = self._dev(t["Bl"]), self._dev(t["c"]), self._dev(t["lp"])
        _lib.call("pm_mix_scores_f64", _ptr(Y), D, _ptr(res["rs"]) if scaled else None, _ptr(Bq_d), _ptr(Bl_d), D, _ptr(c_d),
                  float(t["coef"]), _ptr(lp_d), N, D, H, _ptr(logpj), _ptr(post), self._stream())
        return logpj

    def reconstruct(self, model_params, my_data, device=False, exact=False, variance=False):
        """Posterior-mean denoising: yhat_n = sum_h r_nh W_h with the responsibilities r_nh = pies_h p(y_n | h) / sum_h'
        pies_h' p(y_n | h') of the proper densities of ``log_likelihood`` (MoG with the 1/2; not the reference's E-step
        quirk), for ``my_data['y']`` (host array, torch tensor or DeviceArray).  MoP: in the units of the data its E-step
        sees -- x = y, or the normalised x = s y + 1 when ``A`` is set (W holds rates of x).

        Returns this rank's (my_N, D) float64 rows as a NumPy array, or with ``device=True`` a ``DeviceArray`` left on the
        device; no collective.  A NaN in a data row makes that row NaN and no other; a component with pies_h > 0 whose
        covariance is not positive definite makes every row NaN.  ``model_params`` and the training shard are left as they
        were.  The responsibilities are written as an (N, H) array by pm_recon_expect_f64 (a row softmax in a maximum and a
        sum pass) and multiplied with W by pm_gemm_nt_rows_f64; H within pm_mix_scores_f64's bound for MoG diagonal / MoP.

        ``exact`` is accepted for the component-analysis models' signature: a mixture's posterior mean is exact
        either way, and ``exact=True`` returns the same bits.

        ``variance=True``: returns ``(Yhat, V)``, both NumPy arrays or both ``DeviceArray``, V_nd = sum_h r_nh
        W_dh^2 - yhat_nd^2: the posterior variance of the component mean, the NOISELESS value (the predictive variance of a
        new observation adds the components' own noise, which the caller adds).  ``Yhat`` has the bits of the call without
        the keyword; a value rounding takes below 0 is returned as 0; a NaN row of the data gives a NaN row of V.  One more
        pm_gemm_nt_rows_f64 of the responsibilities against W o W, then pm_recon_var_finish_f64.  Together with
        ``exact=True`` it raises ``NotImplementedError``, as the component-analysis models do."""
        self._refuse_mask(my_data)
        if variance and exact:
            raise NotImplementedError("%s.reconstruct: variance=True with exact=True is not built" % type(self).__name__)
        y = my_data['y']
        N, H, D = int(y.shape[0]), self.H, self.D
        if N == 0:
            empty = lambda: DeviceArray(torch.empty((0, D), dtype=torch.float64, device=self.device)) if device \
                else np.empty((0, D))
            return (empty(), empty()) if variance else empty()
        saved = dict(self.__dict__)
        slot = saved.get("_eval_slot") or {"_data": {}, "_ws": {}}
        self._data, self._ws = slot["_data"], slot["_ws"]
        try:
            res = self._resident(y)
            X, a, off_d = self._recon_scores(dict(model_params), res)
            Kp = (H + 7) // 8 * 8
            r = self._buf("recon_r", (N, Kp))
            one = (ctypes.c_double * 8)(1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
            st = self._stream()
            _lib.call("pm_recon_expect_f64", _ptr(X), H, None, ctypes.c_double(a), _ptr(off_d), None, None, one, N, H, 0, H,
                      0, 1, 0, 0, _ptr(r), Kp, Kp, -1, st)
            Wp = np.zeros((D, Kp))
            Wp[:, :H] = np.asarray(model_params['W'], dtype=np.float64)
            W_d = self._dev(Wp)
            out = torch.empty((N, D), dtype=torch.float64, device=self.device)
            _lib.call("pm_gemm_nt_rows_f64", _ptr(r), Kp, _ptr(W_d), Kp, _ptr(out), D, N, D, Kp, st)
            if variance:
                # (the second moment per component is the responsibility itself: pm_recon_moments2_f64 with one block of
                # value 1 and no table would write ``r`` again)
                V = torch.empty((N, D), dtype=torch.float64, device=self.device)
                _lib.call("pm_gemm_nt_rows_f64", _ptr(r), Kp, _ptr(self._dev(Wp * Wp)), Kp, _ptr(V), D, N, D, Kp, st)
                _lib.call("pm_recon_var_finish_f64", _ptr(V), D, _ptr(out), D, None, None, 1, None, None, D, N, H, D, 0, st)
                return (DeviceArray(out), DeviceArray(V)) if device else (out.cpu().numpy(), V.cpu().numpy())
            return DeviceArray(out) if device else out.cpu().numpy()
        finally:
            slot = {"_data": self._data, "_ws": self._ws}
            self.__dict__.clear()
            self.__dict__.update(saved)
            self._eval_slot = slot

    # ---- latent codes -----------------------------------------------------------------------------------
    def encode(self, model_params, my_data, device=False, exact=False):
        """The code of every datapoint: ``(mean, prob)``, both (my_N, H) float64 and both the responsibilities r_nh = pies_h
        p(y_n | h) / sum_h' pies_h' p(y_n | h') that ``reconstruct`` averages with (the proper densities of
        ``log_likelihood``, from the same scores): the latent of a mixture is one-hot, so E[s_h | y_n] = P(s_h != 0 | y_n).
        NumPy arrays, or with ``device=True`` two ``DeviceArray`` left on the device; no collective.  A NaN in a data row
        makes that row NaN and no other; ``model_params`` and the training shard are left as they were.  ``exact`` is
        accepted for the component-analysis models' signature and returns the same bits; ``my_data['mask']`` and
        ``my_data['weight']`` are refused.  One launch of pm_encode_f64 (a row softmax in a maximum and a sum pass)."""
        self._refuse_mask(my_data)
        y = my_data['y']
        N, H = int(y.shape[0]), self.H
        if N == 0:
            empty = lambda: DeviceArray(torch.empty((0, H), dtype=torch.float64, device=self.device)) if device \
                else np.empty((0, H))
            return empty(), empty()
        saved = dict(self.__dict__)
        slot = saved.get("_eval_slot") or {"_data": {}, "_ws": {}}
        self._data, self._ws = slot["_data"], slot["_ws"]
        try:
            res = self._resident(y)
            X, a, off_d = self._recon_scores(dict(model_params), res)
            mean = torch.empty((N, H), dtype=torch.float64, device=self.device)
            prob = torch.empty((N, H), dtype=torch.float64, device=self.device)
            one = (ctypes.c_double * 8)(1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
            _lib.call("pm_encode_f64", _ptr(X), H, None, ctypes.c_double(a), _ptr(off_d), None, None, one, N, H, 0, H, 0, 1,
                      0, 0, _ptr(mean), H, _ptr(prob), H, self._stream())
            return (DeviceArray(mean), DeviceArray(prob)) if device else (mean.cpu().numpy(), prob.cpu().numpy())
        finally:
            slot = {"_data": self._data, "_ws": self._ws}
            self.__dict__.clear()
            self.__dict__.update(saved)
            self._eval_slot = slot

    # ---- posterior draws --------------------------------------------------------------------------------
    sample_chunk_bytes = 1 << 26      # bound of the workspace beside the result (indices and lists of one row chunk)
    sample_chunk_rows = None          # rows per chunk when set (tests): the draws do not depend on it

    def _sample_posterior(self, model_params, my_data, n_samples, seed, latents, device, uniforms, normals):
        """``MixtureModel.sample_posterior``: the scores of ``reconstruct`` (``_recon_scores``), then per row chunk
        pm_sample_states_f64 (h ~ softmax(a X + o)), pm_sample_active_f64 (one block of value 1, no table) and
        pm_sample_decode_lin_f64 against W^T, written in place."""
        from ..camodels._device import DeviceCAModel
        y = my_data['y']
        N, H, D = int(y.shape[0]), self.H, self.D
        M = DeviceCAModel._sample_check(N, n_samples, uniforms, None)
        self._refuse_mask(my_data)
        wrap = (lambda t: DeviceArray(t)) if device else (lambda t: t.cpu().numpy())
        if N == 0:
            z = lambda c: DeviceArray(torch.empty((M, 0, c), dtype=torch.float64, device=self.device)) if device \
                else np.empty((M, 0, c))
            return (z(D), z(H)) if latents else z(D)
        saved = dict(self.__dict__)
        slot = saved.get("_eval_slot") or {"_data": {}, "_ws": {}}
        self._data, self._ws = slot["_data"], slot["_ws"]
        try:
            res = self._resident(y)
            X, a, off_d = self._recon_scores(dict(model_params), res)
            if uniforms is None:
                g = torch.Generator(device=self.device)
                g.manual_seed(int(seed)) if seed is not None else g.seed()
                U = torch.rand((N, M), generator=g, device=self.device, dtype=torch.float64)
            else:
                U = getattr(uniforms, "tensor", uniforms)
                if not torch.is_tensor(U):
                    U = torch.from_numpy(np.ascontiguousarray(np.asarray(U), dtype=np.float64))
                U = U.to(device=self.device, dtype=torch.float64).contiguous()
            Wt = self._dev(np.asarray(model_params['W'], dtype=np.float64).T)
            Ys = torch.empty((M, N, D), dtype=torch.float64, device=self.device)
            Sl = torch.empty((M, N, H), dtype=torch.float64, device=self.device) if latents else None
            one = (ctypes.c_double * 8)(1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
            st = self._stream()
            rows = max(1, int(self.sample_chunk_rows)) if self.sample_chunk_rows else \
                max(1, min(N, int(self.sample_chunk_bytes) // (M * 16)))
            for n0 in range(0, N, rows):
                n = min(rows, N - n0)
                idx = torch.empty((n, M), dtype=torch.int32, device=self.device)
                ai = torch.empty((n, M, 1), dtype=torch.int32, device=self.device)
                av = torch.empty((n, M, 1), dtype=torch.float64, device=self.device)
                _lib.call("pm_sample_states_f64", ctypes.c_void_p(X.data_ptr() + 8 * n0 * H), H, None, ctypes.c_double(a),
                          _ptr(off_d), ctypes.c_double(0.0), -1, ctypes.c_void_p(U.data_ptr() + 8 * n0 * M), M, n, H, M,
                          _ptr(idx), st)
                _lib.call("pm_sample_active_f64", _ptr(idx), None, None, one, n, M, H, 0, H, 0, 1, 0, 0, 1, _ptr(ai), _ptr(av), st)
                _lib.call("pm_sample_decode_lin_f64", _ptr(ai), _ptr(av), 1, _ptr(Wt), D, None, n, M, H, D,
                          ctypes.c_void_p(Ys.data_ptr() + 8 * n0 * D), D, N * D, st)
                if latents:
                    Sl[:, n0:n0 + n] = DeviceCAModel._sample_scatter(idx, ai, av, H)
            return (wrap(Ys), wrap(Sl)) if latents else wrap(Ys)
        finally:
            slot = {"_data": self._data, "_ws": self._ws}
            self.__dict__.clear()
            self.__dict__.update(saved)
            self._eval_slot = slot

    # ---- E-step -------------------------------------------------------------------------------------------------------
    def _full_factors(self, sig):
        """The full covariances (H, D, D) factored on the device (pm_mix_chol_f64): returns (B, mode, logdet) for
        pm_mix_maha_f64 -- B_h = L_h^-1 and logdet_h from the device for every positive definite component; a component
        the Cholesky rejects (not positive definite) gets the reference's own operations on the host, np.linalg.inv and
        slogdet(...)[1] (MoG.py:249-252), uploaded into its slot with mode 1.  ``self.fallback_components``: those h."""
        H, D = self.H, self.D
        S_d = self._dev(sig)
        Lw = self._buf("chol_L", (H, D, D))
        B = torch.empty((H, D, D), dtype=torch.float64, device=self.device)
        logdet_d = torch.empty(H, dtype=torch.float64, device=self.device)
        status_d = torch.empty(H, dtype=torch.int32, device=self.device)
        _lib.call("pm_mix_chol_f64", _ptr(S_d), D, H, _ptr(Lw), _ptr(B), _ptr(logdet_d), _ptr(status_d), self._stream())
        status = status_d.cpu().numpy()
        logdet = logdet_d.cpu().numpy().copy()
        bad = np.nonzero(status)[0]
        mode = np.zeros(H, dtype=np.int32)
        with np.errstate(all='ignore'):
            for h in bad:
                B[h] = self._dev(np.linalg.inv(sig[h]).T)
                logdet[h] = np.linalg.slogdet(sig[h])[1]
                mode[h] = 1
        self.fallback_components = [int(h) for h in bad]
        return B, torch.from_numpy(mode).to(self.device), logdet

    def _estep_dev(self, y, coef, c, lp, Bl=None, Bq=None, W_rows=None, B=None, mode=None, scaled=True):
        """logpj and posteriors (N, H) on the device.  Bl given: pm_mix_scores_f64 (MoP, or MoG diagonal with Bq);
        else the full-covariance pair pm_mix_maha_f64 + pm_mix_posterior_f64 on W_rows (H, D) and B, mode of
        ``_full_factors``.  ``scaled`` False: the data's row scale (``_rowscale_host``) is not applied."""
        res = self._resident(y)
        Y, H, D = res["Y"], self.H, self.D
        N = Y.shape[0]
        logpj = torch.empty((N, H), dtype=torch.float64, device=self.device)
        post = torch.empty((N, H), dtype=torch.float64, device=self.device)
        if N:
            st = self._stream()
            c_d, lp_d = self._dev(c), self._dev(lp)
            if Bl is not None:
                Bl_d = self._dev(Bl)
                Bq_d = self._dev(Bq) if Bq is not None else None
                rs = res["rs"] if scaled else None
                _lib.call("pm_mix_scores_f64", _ptr(Y), D, _ptr(rs), _ptr(Bq_d), _ptr(Bl_d), D, _ptr(c_d), float(coef),
                          _ptr(lp_d), N, D, H, _ptr(logpj), _ptr(post), st)
            else:
                W_d = self._dev(W_rows)
                S = self._buf("maha", (N, H))
                _lib.call("pm_mix_maha_f64", _ptr(Y), D, _ptr(W_d), _ptr(B), _ptr(mode), N, D, H, _ptr(S), H, st)
                _lib.call("pm_mix_posterior_f64", _ptr(S), H, _ptr(c_d), float(coef), _ptr(lp_d), N, H, _ptr(logpj),
                          _ptr(post), st)
        return {'posteriors_h': DeviceArray(post), 'logpj': DeviceArray(logpj)}

    # ---- M-step -------------------------------------------------------------------------------------------------------
    def _mstats(self, y, posteriors, kind):
        """The packed statistics [colsum P | Y^T P | (Y*Y)^T P or the H Gram matrices] of this shard, summed over ranks
        with ONE all-reduce, on the host.  ``posteriors``: the E-step's device handle or any (N, H) array."""
        res = self._resident(y)
        Y, H, D = res["Y"], self.H, self.D
        N = Y.shape[0]
        L = int(_lib.load().pm_mix_stats_len(D, H, kind))
        if N:
            if isinstance(posteriors, DeviceArray):
                P = posteriors.tensor
            elif torch.is_tensor(posteriors):
                P = posteriors.to(device=self.device, dtype=torch.float64)
            else:
                P = self._dev(np.asarray(posteriors))
            P = P.contiguous()
            assert tuple(P.shape) == (N, H)
            work = self._buf("mstats_work", (int(_lib.load().pm_mix_mstats_work_len(N, D, H, kind)),))
            stats = self._buf("mstats", (L,))
            _lib.call("pm_mix_mstats_f64", _ptr(Y), D, _ptr(P), H, _ptr(res["rs"]) if kind == KIND_MOP else None, N, D, H,
                      kind, _ptr(work), _ptr(stats), self._stream())
            host = stats.cpu().numpy()
        else:
            host = np.zeros(L)
        return self.comm.allreduce(host)
