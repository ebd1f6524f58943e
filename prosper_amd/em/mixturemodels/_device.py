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
        """Forget the resident shard (call after modifying ``my_data['y']`` in place)."""
        self._data = {}

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
