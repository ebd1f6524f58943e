"""What the two table models (DSC_ET, TSC_ET) share on top of the device plumbing: their log-joints have one column per
row of a state table over the H' candidate positions (csrc/dsc_kernels.hip), so the E-step launch, the M-step up to the
all-reduced statistics and the W update from them are one code; a model adds its prior, its cut rule and its pi / sigma
formulas."""
import ctypes

import numpy as np

from ._device import DeviceCAModel, DeviceArray, _ptr, small_blas
from ... import _lib
from ...utils import tracing

try:
    import torch
except Exception:  # pragma: no cover
    torch = None


class TableCAModel(DeviceCAModel):
    """A model supplies: ``_tables()``, ``_params(anneal, pi, sigma)``, ``_prior(pi)``, ``_finalize(stats, model_params,
    *extra)`` and

      _stats_ws, _prior_ws   names of its statistics workspace and its prior upload
      _n_logpj()             columns of ``logpj``
      _prior_factors(mp)     (pi as ``_params`` / ``_prior`` take it, the pi key of ``_dsc_estep`` / ``_dsc_fused_stats``,
                             A_pi_gamma, the arguments of ``_finalize`` behind ``model_params``)
      _cut_rule              (device form, host form): the N_use-th largest log-evidence -> the cut the row pass keeps
                             the datapoints STRICTLY above
    """

    _stats_ws = _prior_ws = _cut_rule = None

    # ---- EM-loop pipelining: the M-step solves W^T on the device, the next step's products follow from it there ----
    def _seed_next(self, res, Wt):
        """Next step's Gram matrix and scores from ``Wt`` = W_new^T (H,D), which the M-step has just solved on the
        device -- enqueued behind the M-step's download so they run while the host unpacks it.  ``_take_seed``
        hands them to the next ``select_Hprimes`` if the caller feeds the returned W back unchanged."""
        Y = res["Y"]
        N, H = Y.shape[0], self.H
        A = self._buf("scores_spec", (N, H))
        if self._par.get("A") is A:
            self._par = {}                 # the cached parameters' scores live in the buffer overwritten now
        G = self._gemm_nt(Wt, Wt, torch.empty((H, H), dtype=torch.float64, device=self.device), "gram_gemm")
        if N:
            self._gemm_nt(Y, Wt, A, "scores_gemm")
        self._seed_rec = {"ykey": res["key"], "Wt": Wt, "G": G, "A": A, "W": None}

    def _scores_params(self, W, res):
        """Device copy of W^T (H,D), the Gram matrix and the scores for the current W and data.  In an EM loop
        the last M-step has left all three on the device (``_seed_next``): W is compared with ITS snapshot first, and once
        per ``step`` -- select_Hprimes, E_step and M_step see the same array object there, and a 256 x 128 comparison costs
        27 us of host time that sits on the loop's critical path (three of them per step until round 4: the device idled
        ~0.1 ms per 0.7 ms iteration waiting for the E-step launch)."""
        W_in = W
        W = np.asarray(W, dtype=np.float64)
        par = self._par
        # The once-per-step shortcut keys on the IDENTITY of the caller's array, so only for an object that is already the
        # float64 ndarray the comparison would read (a converted temporary's id() can be recycled), and the record keeps a
        # reference to it (an id() is only unique among live objects).  Contract: W is not edited in place between
        # select_Hprimes, E_step and M_step of one ``step`` (CAModel.step never does).
        tag = (getattr(self, "_step_id", 0), id(W)) if (getattr(self, "_in_step", False) and W is W_in) else None
        if tag is not None and par.get("checked") == tag and par.get("checked_obj") is W and par.get("ykey") == res["key"]:
            return par
        if getattr(self, "_seed_rec", None) is not None:
            seeded = self._take_seed(W, res)
            if seeded is not None:           # W^T, Gram matrix and scores left on the device by the last M-step
                seeded["checked"], seeded["checked_obj"] = tag, (W if tag is not None else None)
                self._par = seeded
                return seeded
        if par.get("ykey") == res["key"] and par.get("W") is not None and par["W"].shape == W.shape \
                and np.array_equal(par["W"], W):
            par["checked"], par["checked_obj"] = tag, (W if tag is not None else None)
            return par
        Wt = self._upload("W", W).t().contiguous()
        G = self._gemm_nt(Wt, Wt, self._buf("gram", (self.H, self.H)), "gram_gemm")
        Y = res["Y"]
        A = self._buf("scores", (Y.shape[0], self.H))
        if Y.shape[0]:
            self._gemm_nt(Y, Wt, A, "scores_gemm")
        self._par = {"ykey": res["key"], "W": W.copy(), "Wt": Wt, "G": G, "A": A, "checked": tag,
                     "checked_obj": W if tag is not None else None}
        return self._par

    def _take_seed(self, W, res):
        """The seeded parameter record if ``W`` (D,H) is what the last M-step returned (compared with a private
        snapshot, so in-place edits by the caller are seen); the seed is consumed either way."""
        seed, self._seed_rec = getattr(self, "_seed_rec", None), None
        if seed is None or seed["W"] is None or seed["ykey"] != res["key"] or seed["W"].shape != W.shape \
                or not np.array_equal(seed["W"], W):
            return None
        return {"ykey": res["key"], "W": seed["W"], "Wt": seed["Wt"], "G": seed["G"], "A": seed["A"]}

    def _dsc_estep(self, anneal, stats_name, par, res, cand, tab, S, prior, P, Kt, pi_key):
        """DSC / TSC E-step launch.  Inside ``step`` with no data truncation ahead the sixteen-lane kernel also produces the
        M-step's row statistics (pm_dsc_estep_mstats_f64: E[s] rows and their non-zero lists, Wq, qdiag, value counts,
        scalars) from the exponentials its log-sum-exp evaluates anyway -- ``M_step`` then skips its pass over the
        log-joints.  Returns the DeviceArray of log-joints with ``.lse`` and, fused, ``.mstats``."""
        N = res["Y"].shape[0]
        H, D, Hp = self.H, self.D, self.Hprime
        lib = _lib.load()
        logpj = torch.empty((N, Kt), dtype=torch.float64, device=self.device)
        lse = torch.empty((N,), dtype=torch.float64, device=self.device)
        out = DeviceArray(logpj)
        out.lse = lse
        out.mstats = None
        if not N:
            return out
        st = self._stream()
        if self.deterministic:
            self._det_dsc_quanta(res, par, P, prior, Kt)
        fuse = (getattr(self, "_in_step", False) and getattr(self, "fuse_mstats", True) and anneal['Ncut_factor'] <= 0.0
                and bool(lib.pm_dsc_estep_mstats_supported(H, Hp, S, int(P.K), int(P.flags))))
        if fuse:
            stats = self._buf(stats_name, (lib.pm_dsc_stats_len(H, D),))
            stats.zero_()
            expect = self._buf("expect", (N, H))
            nz = None
            if getattr(self, "sparse_wp", True):
                nz = (self._buf("nz_idx", (N, 16), torch.int16), self._buf("nz_val", (N, 16)))
            self._call("estep_mstats", "pm_dsc_estep_mstats_f64", _ptr(par["A"]), H, _ptr(par["G"]), _ptr(res["ynorm2"]),
                       _ptr(cand), _ptr(tab), S, _ptr(prior), ctypes.byref(P), N, H, D, Hp, _ptr(logpj), Kt, _ptr(lse),
                       _ptr(expect), H, _ptr(stats), _ptr(nz[0]) if nz else None, _ptr(nz[1]) if nz else None, st)
            out.mstats = {"stats": stats, "expect": expect, "nz": nz, "res": res, "cand": cand,
                          "P": (float(P.ecoef), float(P.pscale), int(P.flags)), "pi": np.array(pi_key, dtype=np.float64, copy=True)}
        else:
            self._call("estep", "pm_dsc_estep_f64", _ptr(par["A"]), H, _ptr(par["G"]), _ptr(res["ynorm2"]), _ptr(cand),
                       _ptr(tab), S, _ptr(prior), ctypes.byref(P), N, H, Hp, _ptr(logpj), Kt, _ptr(lse), st)
        return out

    def _det_dsc_quanta(self, res, par, P, prior, Kt):
        """Deterministic mode, DSC / TSC: bounds of the statistics' partial sums (latent values v_k, |v| <= vmax) -> quanta of
        the row kernels, the sparse product and the dense GEMM behind its gate (pm_common.h, PM_Q).  Set ahead of the E-step,
        whose parameters the M-step of the same EM step shares."""
        ymax, ynmax = self._det_data_bounds(res)
        W = np.asarray(par["W"], dtype=np.float64)
        wn = float(np.sqrt((W * W).sum(axis=0)).max()) if W.size else 0.0
        vmax = float(max(abs(P.values[k]) for k in range(int(P.K))))
        emax = (ynmax + self.gamma * vmax * wn) ** 2
        lpmax = abs(P.pscale) * float(prior.abs().max()) + abs(P.ecoef) * emax + np.log(max(Kt, 2))
        n = float(res["Y"].shape[0])
        self._det_set("dsc", [n * max(1.0, vmax * vmax), n * emax, n * lpmax])
        self._det_set("wp_sparse", [n * vmax * ymax])
        self._det_set("gemm", [n * max(1.0, vmax) * ymax, n * ymax])

    def _dsc_fused_stats(self, logpj, res, cand, P, pi_key, lse_cut):
        """The statistics workspace the E-step pass has already filled for exactly this M-step, or None."""
        ms = getattr(logpj, "mstats", None) if isinstance(logpj, DeviceArray) else None
        if ms is None:
            return None
        logpj.mstats = None
        if (ms["res"] is res and ms["cand"] is cand and lse_cut == float("-inf")
                and ms["P"] == (float(P.ecoef), float(P.pscale), int(P.flags))
                and np.array_equal(ms["pi"], np.asarray(pi_key, dtype=np.float64))):
            return ms
        return None

    def _rows_and_wp(self, rows_args, lp_ld, expect, Y, stats, my_N, K, flags, Hp, S, fused=None, cut_dev=None):
        """DSC / TSC M-step: the per-datapoint pass (pm_dsc_mstep_rows[_nz]_f64) and Wp = E[s]^T Y.  Where the
        sixteen-lane kernel applies the pass also leaves the non-zero lists of E[s] and Wp is accumulated from them
        (pm_wp_sparse_f64); the dense product follows behind the device-side gate (last scalar of `stats`: rows whose
        list overflowed) and only does work then.  ``fused``: the record of an E-step pass that has already produced the
        row statistics (``_dsc_estep``): only the product is left."""
        H, D = self.H, self.D
        lib = _lib.load()
        st = self._stream()
        gate = ctypes.c_void_p(stats.data_ptr() + 8 * (lib.pm_dsc_stats_len(H, D) - 1))

        def wp(nz):
            if nz is not None:
                self._call("stats_sparse", "pm_wp_sparse_f64", _ptr(nz[0]), _ptr(nz[1]), _ptr(Y), Y.stride(0), _ptr(stats),
                           D, gate, my_N, H, D, st)
                self._call("stats_gemm", "pm_gemm_tn_acc_gated_f64", _ptr(expect), H, _ptr(Y), D, _ptr(stats), D, H, D,
                           my_N, gate, st)
            else:
                self._call("stats_gemm", "pm_gemm_tn_acc_f64", _ptr(expect), H, _ptr(Y), D, _ptr(stats), D, H, D, my_N, st)

        if fused is not None:
            return wp(fused["nz"])
        sparse = (getattr(self, "sparse_wp", True) and Y.is_cuda and H <= 256
                  and bool(lib.pm_dsc_rows16_supported(H, Hp, S, K, flags)))
        nz = (self._buf("nz_idx", (my_N, 16), torch.int16), self._buf("nz_val", (my_N, 16))) if sparse else None
        if cut_dev is not None:
            # ``cut_dev``: the data-truncation cut as the radix select left it on the device (round 6: no host round trip
            # between the select and this pass -- on a slow host the device idled a quarter of the step there)
            rows_args = rows_args[:4] + (_ptr(cut_dev),) + rows_args[4:]
            self._call("mstep_rows", "pm_dsc_mstep_rows_cutp_f64",
                       *(rows_args + ((_ptr(nz[0]), _ptr(nz[1])) if sparse else (None, None)) + (st,)))
        elif sparse:
            self._call("mstep_rows", "pm_dsc_mstep_rows_nz_f64", *(rows_args + (_ptr(nz[0]), _ptr(nz[1]), st)))
        else:
            self._call("mstep_rows", "pm_dsc_mstep_rows_f64", *(rows_args + (st,)))
        wp(nz)

    @tracing.traced
    def M_step(self, anneal, model_params, my_suff_stat, my_data):
        """New W, pi, sigma (dsc_et.py:587-774, tsc_et.py:359-542): the statistics of the kept datapoints, one all-reduce,
        the model's ``_finalize``."""
        self._refuse_training_mask(my_data)
        H, Hp, D = self.H, self.Hprime, self.D
        S, Kt = self.state_matrix.shape[0], self._n_logpj()
        sigma = model_params['sigma']
        res = self._resident(my_data['y'])
        Y = res["Y"]
        my_N = Y.shape[0]
        tab = self._tables()
        cand = self._device_candidates(my_data['candidates'], my_N)

        logpj = my_suff_stat['logpj']
        if isinstance(logpj, DeviceArray) and getattr(logpj, "lse", None) is not None:
            lp, lse = logpj.tensor, logpj.lse
        else:
            lp = torch.from_numpy(np.ascontiguousarray(np.asarray(logpj), dtype=np.float64)).to(self.device)
            lse = torch.logsumexp(lp, dim=1)
        lp, lse = lp.contiguous(), lse.contiguous()
        assert tuple(lp.shape) == (my_N, Kt)
        N = self._global_count(res, my_N)

        pi, pi_key, A_pi_gamma, extra = self._prior_factors(model_params)

        # data truncation (dsc_et.py:825-843, tsc_et.py:435-446)
        lse_cut, cut_dev = float("-inf"), None
        if anneal['Ncut_factor'] > 0.0:
            tracing.tracepoint("M_step:truncating")
            N_use = int(N * (1 - (1 - A_pi_gamma) * anneal['Ncut_factor'])) or N    # (0: upstream's allsort(...)[-0] keeps everything)
            cut_on_device, cut_on_host = self._cut_rule
            if lse.is_cuda and my_N:      # (the cut stays on the device: the row pass reads it there)
                cut_dev = cut_on_device(self._kth_select_dev(lse, N_use))
                lse_cut = float("nan")    # (not -inf: statistics a fused E-step pass may have left do not apply)
            else:
                lse_cut = cut_on_host(self._kth_largest_global(lse, N_use))

        tracing.tracepoint("M_step:iterating")
        lib = _lib.load()
        P = self._params(anneal, pi, sigma)
        fused = self._dsc_fused_stats(logpj, res, cand, P, pi_key, lse_cut) if my_N else None
        stats = fused["stats"] if fused else self._buf(self._stats_ws, (lib.pm_dsc_stats_len(H, D),))
        if not fused:
            stats.zero_()
        expect = self._buf("expect", (my_N, H))
        # (the fused pass has used the prior already; only the M-step's own row pass needs it again)
        prior = None if fused else self._upload(self._prior_ws, self._prior(pi))
        if my_N:
            self._rows_and_wp((_ptr(lp), Kt, _ptr(lse), ctypes.c_double(lse_cut), _ptr(cand), _ptr(tab), S,
                               _ptr(prior) if prior is not None else None,
                               ctypes.byref(P), my_N, H, D, Hp, _ptr(expect), H, _ptr(stats)),
                              Kt, expect, Y, stats, my_N, int(P.K), int(P.flags), Hp, S, fused=fused, cut_dev=cut_dev)
        self.comm.allreduce_device(stats)     # the models' allreduces of Wp, Wq, the counts, sigma and the likelihood in one
        self._mstep_res = res
        return self._finalize(stats, model_params, *extra)

    def _update_W(self, stats, model_params, fallback):
        """The head of a ``_finalize``: the W update from the all-reduced statistics and the one device->host copy.  Returns
        ``(host, W_out)``: host[:8] the value counts, host[8:12] the scalars (sigma sum, evidence sum, kept datapoints, gate)
        and W_out (D, H), ``model_params['W']`` itself where W is not learned.  ``fallback(Wq, Wp)``: the reference's
        host solve (the ``np.linalg.lstsq(Wq, Wp)`` of dsc_et.py:741), for a numerically singular Wq."""
        H, D = self.H, self.D
        o_wq, o_qd = H * D, H * D + H * H
        o_cnt = o_qd + H
        Wp = stats[:o_wq].view(H, D)
        Wq_u = stats[o_wq:o_qd].view(H, H)
        qdiag = stats[o_qd:o_cnt]
        parts = [stats[o_cnt:o_cnt + 8 + 4]]
        learn_W = 'W' in self.to_learn
        if learn_W:
            tracing.tracepoint("M_step:update W")
            X, status, Wq = self._solve_normal_eq(Wq_u, qdiag, Wp.contiguous())
            parts += [status, X.reshape(-1)]
        flat = torch.cat(parts)
        self._seed_rec = None
        res = getattr(self, "_mstep_res", None)
        if flat.is_cuda and learn_W and res is not None and self.speculate:
            host = self._download(flat, then=lambda: self._seed_next(res, X))
        else:
            host = self._download(flat) if flat.is_cuda else flat.numpy()
        if not learn_W:
            return host, np.asarray(model_params['W'])
        ok = self._solve_ok(float(host[12]), float(host[13]))
        redo = self._solve_accurate(float(host[14])) if ok else None
        if redo is not None:    # the device rejected the inverse's warm start: W from the refined solve, seed void
            self._seed_rec = None
            W_new = redo
        elif ok:
            W_new = host[15:15 + H * D].reshape(H, D).copy()
            if self._seed_rec is not None:
                self._seed_rec["W"] = W_new.copy().transpose()   # private snapshot of the W handed back (same memory order: a
                                                                 # contiguous copy and a contiguous comparison)
        else:   # numerically singular Wq
            self._seed_rec = None
            self._winv_prev = None        # never warm-start the next inverse from a rejected one
            with small_blas():
                W_new = fallback(Wq.cpu().numpy(), Wp.cpu().numpy())
        return host, W_new.transpose()
