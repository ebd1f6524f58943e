"""Device plumbing shared by the HIP-backed component-analysis models: resident data shards,
workspace reuse, asynchronous parameter upload, the one device->host copy per M-step, kernel
launch bookkeeping and the NumPy-compatible handles (``DeviceArray``) results are returned in.
PyTorch supplies memory, streams and process groups; every computation on the hot path is a call
into libprosper_hip.so (include/prosper_hip.h)."""
import contextlib
import ctypes
import os

import numpy as np

from . import CAModel
from ... import _lib
from ...utils import parallel

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

try:
    from threadpoolctl import ThreadpoolController as _ThreadpoolController
except Exception:  # pragma: no cover
    _ThreadpoolController = None

_blas_controller = None


class small_blas(object):
    """Host LAPACK on the H x H matrices of an M-step with a handful of threads: on a 256-core GPU
    host OpenBLAS otherwise wakes every core for a 128 x 128 inverse (measured 16 ms instead of 0.2).
    The library scan of threadpoolctl (0.6 ms) is done once per process."""

    def __init__(self, threads=4):
        global _blas_controller
        if _blas_controller is None and _ThreadpoolController is not None:
            w = np.ones((256, 256))
            np.dot(w, w)                             # OpenBLAS builds its thread pool on the first threaded call:
            np.linalg.inv(w + 256 * np.eye(256))     # do that before any limit is in force (else every call rebuilds it)
            _blas_controller = _ThreadpoolController()
        self._ctx = _blas_controller.limit(limits=threads, user_api="blas") if _blas_controller is not None else None

    def __enter__(self):
        if self._ctx is not None:
            self._ctx.__enter__()
        return self

    def __exit__(self, *exc):
        if self._ctx is not None:
            self._ctx.__exit__(*exc)
        return False


class DeviceArray(object):
    """NumPy-compatible handle of a tensor living in HBM.

    ``np.asarray(handle)`` (or any NumPy function) downloads it once; row selection with an
    index array stays on the device (``CAModel.select_partial_data``)."""

    def __init__(self, tensor, np_dtype=None):
        self.tensor = tensor
        self._np_dtype = np.dtype(np_dtype) if np_dtype is not None else None
        self._host = None
        self.lse = None          # log-evidence per row, attached to 'logpj' handles

    @property
    def shape(self):
        return tuple(self.tensor.shape)

    @property
    def ndim(self):
        return self.tensor.dim()

    @property
    def dtype(self):
        if self._np_dtype is not None:
            return self._np_dtype
        return np.dtype(str(self.tensor.dtype).replace("torch.", ""))

    def __len__(self):
        return self.tensor.shape[0]

    def numpy(self):
        if self._host is None:
            host = self.tensor.detach().cpu().numpy()
            if self._np_dtype is not None and host.dtype != self._np_dtype:
                host = host.astype(self._np_dtype)
            self._host = host
        return self._host

    def __array__(self, dtype=None, copy=None):
        a = self.numpy()
        return a.astype(dtype) if dtype is not None and np.dtype(dtype) != a.dtype else a

    def __getitem__(self, idx):
        if isinstance(idx, np.ndarray) and idx.ndim == 1 and idx.dtype.kind in "iub":
            t = torch.from_numpy(np.ascontiguousarray(idx)).to(self.tensor.device)
            out = DeviceArray(self.tensor[t], self._np_dtype)
            if self.lse is not None:
                out.lse = self.lse[t]
            return out
        return self.numpy()[idx]

    def __repr__(self):
        return "DeviceArray(shape=%s, dtype=%s, device=%s)" % (self.shape, self.dtype, self.tensor.device)


class LazyCandidates(DeviceArray):
    """``data['candidates']`` as handed out by the fast path of ``select_Hprimes``: the
    selection is deferred.  If ``E_step`` is called next with the same parameters (what
    ``CAModel.step`` / ``compute_lpj`` do) both stages run as ONE fused pass that overlaps with
    the scores GEMM; if anything looks at the handle first (``np.asarray``, indexing, ``M_step``
    with foreign log-joints) the candidates are computed on the spot.  Either way the values
    are those of bsc_et.py:98-115."""

    def __init__(self, model, ticket, shape):
        self._model = model
        self._ticket = ticket
        self._shape = tuple(shape)
        self._np_dtype = np.dtype(np.int64)
        self._host = None
        self.lse = None

    @property
    def tensor(self):
        if self._ticket["cand"] is None:
            self._model._materialize_candidates(self._ticket)
        return self._ticket["cand"]

    @property
    def pending(self):
        return self._ticket["cand"] is None

    @property
    def shape(self):
        return self._shape

    @property
    def ndim(self):
        return 2

    def __len__(self):
        return self._shape[0]

    def __repr__(self):
        return "LazyCandidates(shape=%s, pending=%s)" % (self._shape, self.pending)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


_LOG_UNDERFLOW = -745.1332191019412      # log(2^-1075): exp() of anything below rounds to 0.0

_DET_QUANTA_SET = {}      # unit -> the quanta last installed in libprosper_hip_det.so's symbols (process-global, like them)


class _AnnealAt(object):
    """Read-only view of a schedule at another position (``LinearAnnealing.__getitem__`` reads ``cur_pos``,
    annealing.py:90-107); ``pos`` None: the schedule as it stands (objects without a position, e.g. a plain mapping)."""

    def __init__(self, anneal, pos):
        self._a, self._pos = anneal, pos

    def __getitem__(self, name):
        a = self._a
        if self._pos is None:
            return a[name]
        old = a.cur_pos
        a.cur_pos = self._pos
        try:
            return a[name]
        finally:
            a.cur_pos = old


class LoglikPoint(dict):
    """The annealing point ``log_likelihood`` evaluates at: T = 1, no prior annealing, no data truncation, all data and no
    parameter noise (every other entry reads 0)."""

    def __init__(self):
        dict.__init__(self, T=1.0, anneal_prior=False, Ncut_factor=0.0, partial=0)

    def __missing__(self, key):
        return 0.0


class KernelTimer(object):
    """HIP-event timing of individual kernel launches on the stream they are enqueued on
    (torch's current stream, which is the one handed to the C ABI).  bench.py attaches one
    to a model to obtain per-kernel average durations inside the timed region."""

    def __init__(self, only=None, stride=1):
        self.events = {}
        self.only = set(only) if only else None    # labels to time (None = all)
        self.stride = max(1, int(stride))          # time every stride-th launch of a label
        self._count = {}

    def launch(self, label, fn):
        n = self._count[label] = self._count.get(label, 0) + 1
        if (self.only is not None and label not in self.only) or (n - 1) % self.stride:
            fn()
            return
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        end.record()
        self.events.setdefault(label, []).append((start, end))

    def summary(self):
        """label -> (launches, average milliseconds); synchronises."""
        torch.cuda.synchronize()
        return {k: (len(v), sum(a.elapsed_time(b) for a, b in v) / len(v)) for k, v in self.events.items()}



class DeviceCAModel(CAModel):
    """CAModel whose select_Hprimes / E_step / M_step run on one MI355X."""

    def __init__(self, D, H, Hprime, gamma, to_learn=['W', 'pi', 'sigma'], comm=parallel.COMM_WORLD,
                 device=None):
        CAModel.__init__(self, D, H, Hprime, gamma, to_learn, comm)
        self._device = device
        self._data = {}          # resident data shard: key, Y, ynorm2
        self._par = {}           # per-step parameter products
        self._ws = {}            # workspaces keyed by name
        self.timer = None        # optional KernelTimer (bench.py)
        # True: every kernel runs from libprosper_hip_det.so (the same sources with -DPM_DETERMINISTIC: addends of the M-step's
        # atomics rounded to a common quantum first, so their sums do not depend on the order they land in -- pm_common.h) and
        # the host takes no shortcut whose operand order varies: two identical EM loops then agree bit for bit.  Opt-in: a few
        # per cent slower, and sums carry the rounding error of their largest entries on all of them.
        self.deterministic = False
        self._pin = {}           # pinned staging buffers for asynchronous parameter uploads
        self._pin_out = {}       # pinned buffers of the device->host copies (one per M-step), by slot
        self.speculate = os.environ.get('PM_SPECULATE', '1') == '1'   # next step's GEMMs behind the M-step download
        self._seed_rec = None    # what _seed_next left on the device for the next select_Hprimes
        self._mstep_res = None   # resident shard of the M-step in progress (for _seed_next)

    def _state_masks(self):
        """uint16 mask per multi-cause state: bit j <=> candidate position j is on."""
        SM = self.state_matrix.astype(np.int64)
        if not SM.size:
            return np.zeros(0, np.uint16)
        return (SM << np.arange(self.Hprime)[None, :]).sum(axis=1).astype(np.uint16)

    def _u16_dev(self, arr):
        """uint16 payloads travel as int16 tensors (same bytes)."""
        arr = np.ascontiguousarray(arr, dtype=np.uint16)
        if not arr.size:
            return torch.zeros(1, dtype=torch.int16, device=self.device)
        return torch.from_numpy(arr.view(np.int16).copy()).to(self.device)

    @property
    def device(self):
        if self._device is None:
            if torch is None or not torch.cuda.is_available():
                raise _lib.HipError("BSC_ET needs a HIP device: the hot path has no CPU fallback")
            self._device = torch.device("cuda", torch.cuda.current_device())
        return torch.device(self._device)

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _call(self, label, entry, *args):
        """Enqueue one C-ABI entry point on the current stream (raises on a bad status)."""
        det = self.deterministic
        if self.timer is None:
            _lib.call(entry, *args, det=det)
        else:
            self.timer.launch(label, lambda: _lib.call(entry, *args, det=det))

    # ---- deterministic reductions (libprosper_hip_det.so) ------------------------------------------------------------
    @staticmethod
    def _magic(bound):
        """1.5 * 2^e with 2^(e-1) >= bound: adding and subtracting it rounds a value to a multiple of 2^(e-52) (PM_Q)."""
        b = float(bound)
        if not np.isfinite(b) or b <= 0.0:
            return 0.0
        return 1.5 * 2.0 ** (int(np.ceil(np.log2(b))) + 1)

    def _det_set(self, unit, bounds):
        """Install the quanta of one kernel family (include/prosper_hip.h: pm_det_set_quanta) ahead of its next launches:
        ``bounds[c]`` = what no partial sum of category c can exceed on this shard with these parameters."""
        vals = tuple([self._magic(b) for b in bounds] + [0.0] * (8 - len(bounds)))
        # (a quantum is a power of two: it moves only when its bound crosses one -- the six uploads per step of a steady EM loop
        # were six small copies on the stream's critical path for values already there.  The cache is per PROCESS, like the
        # symbols: another model's different bounds invalidate it.)
        cache = _DET_QUANTA_SET
        if cache.get(unit) == vals:
            return
        cache[unit] = vals
        M = (ctypes.c_double * 8)(*vals)
        keep = self.__dict__.setdefault("_det_keep", [])
        keep.append(M)
        del keep[:-16]
        _lib.call("pm_det_set_quanta", _lib.DET_UNITS[unit], M, self._stream(), det=True)

    def _det_data_bounds(self, res):
        """(max |y_nd|, max |y_n|) over the resident shard: constants of the data, once per shard."""
        b = res.get("det_bounds")
        if b is None:
            Y = res["Y"]
            b = res["det_bounds"] = ((float(Y.abs().max()), float(res["ynorm2"].max().sqrt())) if Y.shape[0] else (0.0, 0.0))
        return b

    def _anneal_point(self, anneal):
        """What of an annealing point decides the inputs of an E-step: temperature, prior annealing, truncation, partial
        data, and the parameter noise of ``noisify_params`` (prosper/em/__init__.py:63-107)."""
        return (anneal['T'], bool(anneal['anneal_prior']), anneal['Ncut_factor'], anneal['partial']) + \
            tuple(anneal[p + '_noise'] for p in sorted(self.noise_policy))

    def _predict_anneal(self, anneal):
        """The annealing point of the NEXT ``step`` -- what the M-step launches the next E-step with (_speculate_estep) -- or
        None when it is not known.  A schedule is a pure function of its position (annealing.py:90-107; ``next`` ignores the
        gain and always accepts, :116-130), so for a ``LinearAnnealing`` it is read at ``cur_pos + 1``; but only a
        predictor that was RIGHT about the current step is trusted (a caller that does not advance the schedule between
        steps gets the flat predictor: same point again), nothing is predicted past the schedule's end, and a next step
        with parameter noise or partial data has inputs nobody knows yet.  A wrong prediction costs a dropped pass, never a
        wrong result (E_step compares the scalars the pass was launched with)."""
        sig = self._anneal_point(anneal)
        prev_sig, prev_peek = getattr(self, "_sig_hist", (None, None))
        peek, end = None, False
        cur, steps = getattr(anneal, "cur_pos", None), getattr(anneal, "steps", None)
        if isinstance(cur, int) and isinstance(steps, int):
            if cur + 1 >= steps:
                end = True
            else:
                peek = _AnnealAt(anneal, cur + 1)
        nxt = None
        if not end:
            if peek is not None and prev_peek is not None and sig == prev_peek:
                nxt = peek
            elif sig == prev_sig:
                nxt = peek if (peek is not None and self._anneal_point(peek) == sig) else _AnnealAt(anneal, cur)
        self._sig_hist = (sig, self._anneal_point(peek) if peek is not None else None)
        self._flat_schedule = (sig == prev_sig)
        if nxt is not None:
            nsig = self._anneal_point(nxt)
            if nsig[3] not in (0, 1) or any(nsig[4:]):
                nxt = None
        return nxt

    def step(self, anneal, model_params, my_data):
        """CAModel.step (camodels/__init__.py:163-193); the E-step knows that the M-step follows with the same arguments."""
        if self.exact:
            return self.exact_step(anneal, model_params, my_data)
        self._refuse_training_mask(my_data)
        was, self._in_step = getattr(self, "_in_step", False), True
        self._step_id = getattr(self, "_step_id", 0) + 1
        try:
            return CAModel.step(self, anneal, model_params, my_data)
        finally:
            self._in_step = was

    def _plain_step(self, anneal, model_params, my_data):
        """CAModel.step with none of the bookkeeping the unmasked EM loop keeps between its steps."""
        return CAModel.step(self, anneal, model_params, my_data)

    def _buf(self, name, shape, dtype=None):
        """Reusable device workspace (no allocation inside the EM loop once warm)."""
        dtype = dtype or torch.float64
        t = self._ws.get(name)
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype:
            t = torch.empty(shape, dtype=dtype, device=self.device)
            self._ws[name] = t
        return t

    @staticmethod
    def _probe(y):
        """Cheap fingerprint of a host array (sum over ~16 evenly spaced rows): catches most in-place edits of an
        array that is already resident; ``invalidate_data()`` is the contract for the rest."""
        n = y.shape[0]
        return float(y[::max(1, n // 16)].sum()) if n else 0.0

    def _resident(self, y):
        """Device copy of the data shard + |y_n|^2, uploaded once and kept in HBM.  A shard is recognised by the
        IDENTITY of the caller's array (the record holds a reference, so its address cannot be recycled for
        another array -- ``select_partial_data`` builds a fresh ``y[sel]`` every step); tensors also by their
        version counter, host arrays by a strided fingerprint."""
        src = y
        if isinstance(y, DeviceArray):
            y = y.tensor
        d = self._data
        if d and d.get("src") is src:
            if torch.is_tensor(y):
                if d["ver"] == (y._version, tuple(y.shape)):
                    return d
            elif isinstance(y, np.ndarray) and d["ver"] == (self._probe(y), y.shape):
                return d
        if torch.is_tensor(y):
            ver = (y._version, tuple(y.shape))
            Y = y.to(device=self.device, dtype=torch.float64).contiguous()
        else:
            y = np.asarray(y)
            ver = (self._probe(y), y.shape)
            Y = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float64)).to(self.device)
        N, D = Y.shape
        assert D == self.D
        yn = torch.empty(N, dtype=torch.float64, device=self.device)
        if N:
            self._call("row_sqnorm", "pm_row_sqnorm_f64", _ptr(Y), D, N, D, _ptr(yn), self._stream())
        self._data_gen = getattr(self, "_data_gen", 0) + 1
        self._data = {"key": ("shard", self._data_gen), "src": src, "ver": ver, "Y": Y, "ynorm2": yn}
        self._par = {}
        return self._data

    def _global_count(self, res, my_N):
        """N = sum of the shard sizes (``comm.allreduce(my_N)``, bsc_et.py:225): fetched once per resident
        data set -- on an nccl-only group every host-side allreduce is a blocking device round trip."""
        if res.get("N_global") is None:
            res["N_global"] = self.comm.allreduce(my_N)
        return res["N_global"]

    def _data_moments(self, data):
        """Per-dimension mean and variance of the (sharded) data on the device: two passes over the
        resident shard (pm_col_moments_f64) and two tiny all-reduces, instead of the reference's two
        host passes over N x D (``parallel.allmean``, camodels/__init__.py:209-213)."""
        res = self._resident(data['y'])
        Y = res["Y"]
        my_N, D = Y.shape
        N = self._global_count(res, my_N)
        s1 = torch.zeros(D, dtype=torch.float64, device=self.device)
        if my_N:
            self._call("col_moments", "pm_col_moments_f64", _ptr(Y), Y.stride(0), my_N, D, None, _ptr(s1), self._stream())
        self.comm.allreduce_device(s1)
        mean = s1 / N
        s2 = torch.zeros(D, dtype=torch.float64, device=self.device)
        if my_N:
            self._call("col_moments", "pm_col_moments_f64", _ptr(Y), Y.stride(0), my_N, D, _ptr(mean), _ptr(s2), self._stream())
        self.comm.allreduce_device(s2)
        host = self._download(torch.cat([mean, s2 / N]), slot="moments").copy()
        return host[:D], host[D:]

    def standard_init(self, data):
        """W = data mean + N(0, (sigma_init/4)^2) per column, sigma = mean per-dimension std, pi = 1/H
        (camodels/__init__.py:196-235); the two passes over the data run on the device."""
        W_mean, sigma_sq = self._data_moments(data)
        D = W_mean.shape[0]
        assert D == self.D
        sigma_init = np.sqrt(sigma_sq).sum() / D
        W_init = W_mean[:, None] + np.random.normal(scale=sigma_init / 4., size=[D, self.H])
        return {'W': W_init, 'pi': 1. / self.H, 'sigma': sigma_init}

    # ------------------------------------------------------------------ data generation on the device
    def generate_data(self, model_params, my_N, device=False, seed=None):
        """``device=False``: the reference's host generator, same NumPy RNG stream (camodels/__init__.py:104-122 and
        the models' own versions).  ``device=True``: the same distribution drawn on the GPU (Philox streams of a
        ``torch.Generator``; ``seed`` makes it reproducible) -- the reference's generators are Python loops over
        datapoints (minutes at the sizes of BASELINE configs 3 / 5); returns ``DeviceArray`` handles."""
        if not device:
            return self._generate_data_host(model_params, my_N)
        return self.generate_data_device(model_params, my_N, seed)

    def _generate_data_host(self, model_params, my_N):
        return CAModel.generate_data(self, model_params, my_N)

    def _gen(self, seed):
        g = torch.Generator(device=self.device)
        if seed is None:
            g.seed()
        else:
            g.manual_seed(int(seed))
        return g

    def _mix_linear(self, S, W_DH):
        """y = S . W^T for latent values S (N,H) f64 on the device and W (D,H): the f64 MFMA GEMM of the hot path."""
        W = torch.from_numpy(np.ascontiguousarray(np.asarray(W_DH, dtype=np.float64))).to(self.device)      # (D,H)
        y = torch.empty((S.shape[0], W.shape[0]), dtype=torch.float64, device=self.device)
        if S.shape[0]:
            self._gemm_nt(S.contiguous(), W, y, "generate_gemm")
        return y

    def _draw_latents(self, model_params, my_N, g):
        """Binary latents, P(s_h = 1) = pi (scalar or per latent) -> (N,H) bool on the device."""
        pi = torch.as_tensor(np.asarray(model_params['pi'], dtype=np.float64)).to(self.device)
        return torch.rand((my_N, self.H), generator=g, device=self.device, dtype=torch.float64) < pi

    def _superpose(self, model_params, s, g):
        """Noise-free data for latents ``s`` (N,H) on the device; the linear superposition s . W^T here, models with
        another combination rule override it."""
        return self._mix_linear(s.to(torch.float64), model_params['W'])

    def generate_data_device(self, model_params, my_N, seed=None, noise_on=True):
        g = self._gen(seed)
        s = self._draw_latents(model_params, my_N, g)
        y = self._superpose(model_params, s, g)
        if noise_on:
            y += float(model_params['sigma']) * torch.randn(y.shape, generator=g, device=self.device, dtype=torch.float64)
        return {'y': DeviceArray(y), 's': DeviceArray(s)}

    def invalidate_data(self):
        """Forget the resident shards, the training one and the one of ``log_likelihood`` (call after modifying
        ``my_data['y']`` in place, or to release the held-out data's device memory and workspaces)."""
        self._data = {}
        self._par = {}
        self.__dict__.pop("_eval_slot", None)

    def _gemm_nt(self, A, B, out, label="gemm_nt"):
        M, K = A.shape
        N = B.shape[0]
        # small outputs (Gram matrices, the H x H x D solve products): the deterministic one-workgroup-per-tile kernel --
        # every rank holding the same operands gets the same bits, and no zero fill + K-slice atomics
        fn = "pm_gemm_nt_small_f64" if (M <= 512 and N <= 512) else "pm_gemm_nt_f64"
        if getattr(self, "_rows_gemm", False):
            # reconstruct: one kernel whatever the shape, so that a row of the product is the same bits in a
            # whole array and in a shard of it (the two above pick kernels and K-slices by the number of rows)
            fn = "pm_gemm_nt_rows_f64"
        # (a matrix of ONE row reports whatever stride its history left -- (D, 1).t().contiguous() keeps (1, 1): H = 1 -- and
        # any leading dimension >= its row length describes it)
        ld = lambda t, cols: t.stride(0) if t.shape[0] > 1 else max(int(t.stride(0)), int(cols))
        self._call(label, fn, _ptr(A), ld(A, K), _ptr(B), ld(B, K), _ptr(out), ld(out, N), M, N, K, self._stream())
        return out

    def _upload(self, name, host, keep=False):
        """Asynchronous host -> device copy through a rotating pair of pinned staging buffers
        (a pageable ``.to(device)`` would block the host until the stream drains and stall the
        EM loop at every step boundary).  ``keep``: also return the staging buffer's NumPy view,
        which stays intact until the second-next upload under the same name."""
        slot = self._pin.setdefault(name, {"i": 0, "bufs": [None, None], "evs": [None, None]})
        i = slot["i"] = slot["i"] ^ 1
        buf = slot["bufs"][i]
        if buf is None or buf.shape != host.shape:
            buf = slot["bufs"][i] = torch.empty(host.shape, dtype=torch.float64).pin_memory()
        elif slot["evs"][i] is not None:
            slot["evs"][i].synchronize()          # the copy that last used this buffer has completed
        view = buf.numpy()
        view[...] = host
        dev = torch.empty(host.shape, dtype=torch.float64, device=self.device)
        dev.copy_(buf, non_blocking=True)
        ev = slot["evs"][i] = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        return (dev, view) if keep else dev

    def _download_async(self, flat, slot):
        """Device -> pinned host copy on the copy stream, behind what the main stream holds NOW.  Returns (NumPy view,
        event to ``synchronize()`` on before reading it)."""
        n = flat.numel()
        buf = self._pin_out.get(slot)
        if buf is None or buf.numel() < n:
            buf = self._pin_out[slot] = torch.empty(n, dtype=torch.float64).pin_memory()
        cs = getattr(self, "_copy_stream", None)
        if cs is None:
            cs = self._copy_stream = torch.cuda.Stream(device=self.device)
        cs.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(cs):
            buf[:n].copy_(flat, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(cs)
        return buf[:n].numpy(), ev

    def _download(self, flat, slot="default", then=None):
        """Device -> pinned host copy + wait; returns a NumPy view valid until the next call
        with the same ``slot``.  ``then()`` runs after the copy is enqueued and before the wait:
        work it launches keeps the device busy while the host digests the result."""
        n = flat.numel()
        buf = self._pin_out.get(slot)
        if buf is None or buf.numel() < n:
            buf = self._pin_out[slot] = torch.empty(n, dtype=torch.float64).pin_memory()
        dst = buf[:n]
        main = torch.cuda.current_stream(self.device)
        if then is not None:
            # the copy goes to a stream of its own: what ``then`` enqueues on the main stream (the next step's
            # speculative GEMMs) starts at once instead of queueing behind ~50 us of copy and launch gaps
            cs = getattr(self, "_copy_stream", None)
            if cs is None:
                cs = self._copy_stream = torch.cuda.Stream(device=self.device)
            cs.wait_stream(main)
            with torch.cuda.stream(cs):
                dst.copy_(flat, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(cs)
            then()
        else:
            dst.copy_(flat, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(main)
        ev.synchronize()
        return dst.numpy()

    def _invert_normal_matrix(self, Wq_u, qdiag, status=None):
        """Wq = triu(Wq_u) + triu(Wq_u, 1)^T + diag(qdiag) and its inverse, enqueued on the CURRENT stream:
        ``(Wq, Winv, status)`` -- one-workgroup SPD inverse (csrc/spd_inverse.hip) instead of ~40 rocSOLVER launches.
        Only for device tensors with H <= 256.  ``status`` (3 doubles; ``status``: where to put them, e.g. a slice of the
        caller's download buffer) = [smallest pivot, largest pivot, accurate]: see ``_solve_normal_eq``.
        From the second call on the previous call's inverse warm-starts a Newton-Schulz refinement
        (pm_spd_inverse_warm_f64: ~40 us instead of the sweep's 0.3 ms when the matrix has moved little -- an EM loop;
        the device falls back to the sweep by itself otherwise and says so in status[2]).  ``PM_WARM_INVERSE=0`` disables it."""
        H = qdiag.shape[0]
        Wq = torch.empty((H, H), dtype=torch.float64, device=Wq_u.device)
        Winv = torch.empty((H, H), dtype=torch.float64, device=Wq_u.device)
        prev = getattr(self, "_winv_prev", None)
        warm = (prev is not None and tuple(prev.shape) == (H, H) and prev.device == Wq_u.device
                and os.environ.get("PM_WARM_INVERSE", "1") == "1")
        if warm:
            piv = status if status is not None else torch.empty(3, dtype=torch.float64, device=Wq_u.device)
            work = self._buf("spd_warm_work", (int(_lib.load().pm_spd_inverse_warm_work_len(H)),))
            # (pivots[2] <- the device's own verdict on the warm start: 1 / 2 = refinement accepted, 0 = the sweep ran)
            # The LONG form (scaled start, eight + one steps, ~60 us) where the start is likely to be far: the step after
            # one whose start was (``_warm_long``: _solve_accurate), and data-truncation steps, whose kept set can jump
            # (``_warm_force_long``, set by the model's M_step) -- the short form would hand those to the 0.3 ms sweep.
            # (Measured and dropped: the long form on truncation steps only while a far start is recent.  On the ramp the start
            # residual has norm ~0.08 in every direction: R_0^8 lands at 2-3e-8 in the Frobenius norm, just above the short
            # form's guard, and the step pays the sweep -- the schedule's mean went 2.43 -> 2.49 ms.)
            long = getattr(self, "_warm_long", False) or getattr(self, "_warm_force_long", False)
            self._call("spd_inverse", "pm_spd_inverse_warm_long_f64" if long else "pm_spd_inverse_warm_f64", _ptr(Wq_u), H,
                       _ptr(qdiag), H, _ptr(prev), H, _ptr(work), _ptr(Wq), _ptr(Winv), H, _ptr(piv), self._stream())
        else:
            if status is not None:
                piv = status
                piv[2:] = 1.0
            else:
                piv = torch.ones(3, dtype=torch.float64, device=Wq_u.device)
            self._call("spd_inverse", "pm_spd_inverse_f64", _ptr(Wq_u), H, _ptr(qdiag), H, _ptr(Wq), _ptr(Winv),
                       H, _ptr(piv), self._stream())
        self._winv_was_warm = warm
        self._winv_prev = Winv
        return Wq, Winv, piv

    def _one(self, device):
        one = getattr(self, "_one_dev", None)
        if one is None or one.device != device:
            one = self._one_dev = torch.ones(1, dtype=torch.float64, device=device)
        return one

    def _apply_inverse(self, Wq, Winv, rhs, refine=True, out=None):
        """X = Winv . rhs with one step of iterative refinement, X += Winv (rhs - Wq X) -- skipped (``refine=False``) behind
        the warm-started inverse, whose four Newton-Schulz steps already leave ||I - Wq Winv|| at rounding level.  Products
        run on the deterministic small-GEMM kernel (pm_gemm_nn_small_f64: fixed summation order, no zero fill, no
        K-slice atomics), so ranks that solve the same all-reduced system stay bitwise identical.  ``out``: where X goes."""
        H, D = rhs.shape
        st = self._stream()
        X = out if out is not None else torch.empty((H, D), dtype=torch.float64, device=rhs.device)
        nn = lambda A, B, C: self._call("solve_gemm", "pm_gemm_nn_small_f64", _ptr(A), A.stride(0), _ptr(B), B.stride(0),
                                        _ptr(C), C.stride(0), A.shape[0], B.shape[1], A.shape[1], st)
        if not refine:
            nn(Winv, rhs, X)                 # (Winv is symmetric)
            return X
        X0 = torch.empty((H, D), dtype=torch.float64, device=rhs.device)
        T = torch.empty((H, D), dtype=torch.float64, device=rhs.device)
        nn(Winv, rhs, X0)
        nn(Wq, X0, T)
        R = rhs - T
        nn(Winv, R, T)
        torch.add(X0, T, out=X)
        return X

    def _solve_normal_eq(self, Wq_u, qdiag, rhs, pre=None, out=None, status=None):
        """X = Wq^-1 . rhs, enqueued on the device, for the symmetric second-moment matrix
        Wq = triu(Wq_u) + triu(Wq_u, 1)^T + diag(qdiag) -- the models' ``np.linalg.lstsq(Wq, Wp)``
        (bsc_et.py:380; the table models': camodels/_table.py).  Returns (X (H,D), status (3,) = [smallest, largest pivot of
        the elimination -- smallest <= 0 marks a failed factorisation --, accurate], Wq (H,H)); the caller fetches the status
        with its one download, checks the pivots (``_solve_ok``: "singular" -> LAPACK's lstsq on the host) and hands status[2] to
        ``_solve_accurate``.  ``pre``: the result of ``_invert_normal_matrix`` when the caller has already run it;
        ``out`` / ``status``: device tensors to write X / the status into (slices of the caller's download buffer)."""
        H, D = rhs.shape
        self._last_solve = None
        if rhs.is_cuda and H <= 256:
            Wq, Winv, piv = pre if pre is not None else self._invert_normal_matrix(Wq_u, qdiag, status)
            warm = getattr(self, "_winv_was_warm", False)
            # (after a rejected warm start the next one is likely to be rejected too -- the first EM steps, a jump in the
            # annealing schedule --: refine right away then instead of finding out from the download and repeating the solve)
            refine = (not warm) or getattr(self, "_refine_next", False)
            X = self._apply_inverse(Wq, Winv, rhs, refine=refine, out=out)
            if not refine:
                # The refinement pass of the solve was skipped on the HOST's guess that the device would accept the warm
                # start.  The device's verdict rides behind the pivots; a caller that reads "sweep ran" there repeats the
                # solve with the refinement (_solve_accurate): the accuracy of W no longer depends on the call history.
                self._last_solve = (Wq, Winv, rhs)
            return X, piv, Wq
        if rhs.is_cuda:
            # H > 256: the one-workgroup inverse on 256-blocks + Schur complements (the library's own GEMMs; no rocSOLVER)
            Wq = torch.triu(Wq_u, 1)
            Wq = (Wq + Wq.t() + torch.diag(torch.diagonal(Wq_u) + qdiag)).contiguous()
            Winv, pmin, pmax = self._spd_inverse_blocked(Wq)
            piv = torch.stack([pmin, pmax, self._one(rhs.device)[0]])
            if status is not None:
                status.copy_(piv)
            return self._apply_inverse(Wq, Winv, rhs, out=out), piv, Wq
        # host tensors: the world_size-2 gloo tests feed CPU statistics through the same finalize code (never the
        # product path, whose statistics live on the device)
        Wq = torch.triu(Wq_u, 1)
        Wq = Wq + Wq.t() + torch.diag(torch.diagonal(Wq_u) + qdiag)
        Lc, info = torch.linalg.cholesky_ex(Wq)
        d = torch.diagonal(Lc) ** 2                       # squared Cholesky diagonal = the elimination's pivots
        X = torch.cholesky_solve(rhs, Lc).contiguous()    # garbage if the factorisation failed
        piv = torch.stack([torch.where(info.reshape(()) == 0, d.min(), -torch.ones((), dtype=d.dtype, device=d.device)),
                           d.max(), torch.ones((), dtype=d.dtype, device=d.device)])
        if out is not None:
            out.copy_(X)
            X = out
        if status is not None:
            status.copy_(piv)
        return X, piv, Wq

    def _solve_accurate(self, flag):
        """``None`` if the solution `_solve_normal_eq` returned is at full accuracy -- the refined cold solve, or the warm
        start the device accepted (``flag`` = status[2] from the download: 1) -- else (the device rejected the warm start and
        ran the sweep, but the host had skipped the refinement pass) the refined solution X (H,D) as a host array, computed
        now from the sweep's inverse: X0 + Winv (rhs - Wq X0), exactly what the cold path returns."""
        last, self._last_solve = getattr(self, "_last_solve", None), None
        self._refine_next = (flag == 0.0)
        self._warm_long = (flag != 1.0)       # (a far start this time: the scaled long form next time)
        if flag != 0.0 or last is None:
            return None
        Wq, Winv, rhs = last
        self._redo_dev = self._apply_inverse(Wq, Winv, rhs, refine=True)      # (kept: callers seed the next step from it)
        return self._redo_dev.cpu().numpy()

    def _spd_inverse_blocked(self, A):
        """Inverse of a symmetric positive definite device matrix of any size from pm_spd_inverse_f64 (n <= 256, one
        workgroup) by recursive 2 x 2 blocking:  with T = A11^-1 A12 and the Schur complement S = A22 - A12^T T,
            A^-1 = [[A11^-1 + T S^-1 T^T, -T S^-1], [-S^-1 T^T, S^-1]].
        Returns (inverse, smallest pivot, largest pivot) -- the pivots of the blocks ARE the pivots of the unblocked
        elimination (first those of A11, then those of S).  Products go through pm_gemm_tn_acc_f64 / pm_gemm_nt_f64."""
        n = A.shape[0]
        dev = A.device
        st = self._stream()
        if n <= 256:
            A = A.contiguous()
            inv = torch.empty((n, n), dtype=torch.float64, device=dev)
            piv = torch.empty(2, dtype=torch.float64, device=dev)
            self._call("spd_inverse", "pm_spd_inverse_f64", _ptr(A), n, None, n, None, _ptr(inv), n, _ptr(piv), st)
            return inv, piv[0], piv[1]
        n1 = min(256, n // 2 // 16 * 16) if n <= 512 else (n // 2 + 15) // 16 * 16
        n2 = n - n1
        A11, A12, A22 = A[:n1, :n1].contiguous(), A[:n1, n1:].contiguous(), A[n1:, n1:].contiguous()
        I11, p1min, p1max = self._spd_inverse_blocked(A11)
        T = torch.zeros((n1, n2), dtype=torch.float64, device=dev)
        self._call("solve_gemm", "pm_gemm_tn_acc_f64", _ptr(I11), n1, _ptr(A12), n2, _ptr(T), n2, n1, n2, n1, st)   # I11^T A12
        C = torch.zeros((n2, n2), dtype=torch.float64, device=dev)
        self._call("solve_gemm", "pm_gemm_tn_acc_f64", _ptr(A12), n2, _ptr(T), n2, _ptr(C), n2, n2, n2, n1, st)     # A12^T T
        S = A22 - C
        S = (0.5 * (S + S.t())).contiguous()
        IS, p2min, p2max = self._spd_inverse_blocked(S)
        B12 = torch.empty((n1, n2), dtype=torch.float64, device=dev)
        self._gemm_nt(T, IS, B12, "solve_gemm")                  # T S^-1 (S^-1 symmetric)
        TST = torch.empty((n1, n1), dtype=torch.float64, device=dev)
        self._gemm_nt(B12, T, TST, "solve_gemm")                 # T S^-1 T^T
        out = torch.empty((n, n), dtype=torch.float64, device=dev)
        B11 = I11 + TST
        out[:n1, :n1] = 0.5 * (B11 + B11.t())
        out[:n1, n1:] = -B12
        out[n1:, :n1] = -B12.t()
        out[n1:, n1:] = IS
        return out, torch.minimum(p1min, p2min), torch.maximum(p1max, p2max)

    @staticmethod
    def _solve_ok(piv_min, piv_max):
        """The pivots of ``_solve_normal_eq`` describe a usable solution (positive definite, ratio above 1e-11)."""
        ratio = piv_min / piv_max if piv_max != 0 else 0.0
        return piv_min > 0 and np.isfinite(ratio) and ratio > 1e-11

    def _device_candidates(self, cand, N):
        if isinstance(cand, DeviceArray):
            t = cand.tensor
        else:
            t = torch.from_numpy(np.ascontiguousarray(cand, dtype=np.int32)).to(self.device)
        if t.dtype != torch.int32:
            t = t.to(torch.int32)
        assert tuple(t.shape) == (N, self.Hprime)
        return t.contiguous()

    KTH_ROUNDS = ((52, 12), (40, 12), (28, 12), (16, 12), (4, 12), (0, 4))     # (shift, bits) of the radix digits

    def _kth_largest_global(self, lse, N_use):
        """sort(all log-evidences over all ranks)[-N_use] (bsc_et.py:252 via parallel.allsort) by distributed radix
        select (csrc/kth_select.hip): per round one histogram pass over the local shard, ONE all-reduce of 4096 bins
        (32 KB, instead of gathering 8 N bytes to every rank and sorting them there), a one-workgroup scan; six rounds
        decide all 64 bits of the order statistic, so the value is exactly the one a full sort returns.  Only the
        final double reaches the host.  (CPU tensors -- the gloo tests -- walk the same protocol with torch ops.)"""
        comm = self.comm
        lse = lse.contiguous()
        dev = lse.device
        n = int(lse.shape[0])
        if lse.is_cuda:
            return float(self._kth_select_dev(lse, N_use).item())
        state = torch.zeros(2, dtype=torch.int64, device=dev)
        state[1] = int(N_use)
        hist = torch.zeros(4096, dtype=torch.int64, device=dev)
        # host tensors (tests): the same rounds on the same 64-bit keys
        b = lse.view(torch.int64)
        key = torch.where(b < 0, ~b, b | torch.iinfo(torch.int64).min)          # order-preserving as UNSIGNED 64-bit
        ukey = key.numpy().view(np.uint64)
        prefix, k = np.uint64(0), int(N_use)
        for shift, bits in self.KTH_ROUNDS:
            top = shift + bits
            match = np.ones(n, dtype=bool) if top >= 64 else ((ukey >> np.uint64(top)) == (prefix >> np.uint64(top)))
            digit = ((ukey[match] >> np.uint64(shift)) & np.uint64((1 << bits) - 1)).astype(np.int64)
            hist = torch.from_numpy(np.bincount(digit, minlength=4096).astype(np.int64))
            comm.allreduce_device(hist)
            h = hist.numpy()
            above = 0
            for d in range((1 << bits) - 1, -1, -1):
                if above + int(h[d]) >= k:
                    break
                above += int(h[d])
            prefix |= np.uint64(d) << np.uint64(shift)
            k -= above
        bits64 = (prefix & np.uint64(0x7FFFFFFFFFFFFFFF)) if (prefix >> np.uint64(63)) else ~prefix
        return float(np.array([bits64], dtype=np.uint64).view(np.float64)[0])

    def _kth_select_dev(self, lse, N_use):
        """The radix select of ``_kth_largest_global`` on a device tensor, result LEFT ON THE DEVICE (one double): the
        deferred statistics of a data-truncation step (pm_bsc_defer_apply_f64) read the cut from there, so the step has no
        host round trip between its E-step pass and its M-step kernels."""
        comm = self.comm
        lse = lse.contiguous()
        dev = lse.device
        n = int(lse.shape[0])
        # one persistent buffer [states: 7 x (prefix, k) | pad | 6 histograms of 4096 bins], zeroed when it is allocated and
        # left zeroed by every select's final kernel; the rank travels as an argument of round 0: 6 + 1 launches, no fills
        ws = self.__dict__.get("_kth_buf")
        if ws is None or ws[0].device != dev or ws[1]:
            ws = self._kth_buf = [torch.zeros(16 + 6 * 4096, dtype=torch.int64, device=dev), False]
        ws[1] = True                   # (dirty until the final kernel is enqueued: an exception in between re-zeroes)
        buf = ws[0]
        states, hists = buf[:14], buf[16:].view(6, 4096)
        st = self._stream()
        prev = (0, 1)
        for r, (shift, bits) in enumerate(self.KTH_ROUNDS):
            if r and comm.size > 1:
                comm.allreduce_device(hists[r - 1])
            self._call("kth_round", "pm_kth_round_k_f64", _ptr(lse) if n else None, n, _ptr(states), _ptr(hists), r, prev[0],
                       prev[1], shift, bits, int(N_use) if r == 0 else -1, st)
            prev = (shift, bits)
        if comm.size > 1:
            comm.allreduce_device(hists[len(self.KTH_ROUNDS) - 1])
        out = torch.empty(1, dtype=torch.float64, device=dev)
        self._call("kth_final", "pm_kth_final_z_f64", _ptr(states), _ptr(hists), len(self.KTH_ROUNDS), prev[0], prev[1],
                   _ptr(out), 1, st)
        ws[1] = False
        return out

    # ------------------------------------------------------------------ inference ("next" row)
    def _adaptive_inference(self, anneal, model_params, test_data, topK, adaptive, Hprime_max, gamma_max,
                            run_pass, regenerate, restore):
        """The loop every model's ``inference`` runs (camodels/__init__.py:256-375): log-joints of the datapoints still in
        play from ``compute_lpj``, one pass of the model's top-K kernel over them, and with ``adaptive`` the datapoints whose
        MAP state has exactly gamma active units again with Hprime+1 / gamma+1 until none remain or the caps are reached.

        ``run_pass(lp, cd, k_eff, ind_n, buf)``: launch the model's pm_infer_topk* kernel on the (n, K) log-joints ``lp`` and
        the (n, Hprime) int64 candidates ``cd``, hand the ranked state indices to ``_refuse_nan`` and write rows ``ind_n`` of
        ``buf['s']`` (first ``k_eff`` entries), ``buf['m']`` and ``buf['p']``.  ``regenerate()``: the model's state tables
        for the grown ``self.Hprime`` / ``self.gamma``; ``restore()``: what the model does once both are back at their
        starting values, whatever happened.  Returns ``buf``: device tensors ``s`` (N,topK,H) int8, ``m`` (N,H), ``p``
        (N,topK), ``gamma`` and ``Hprime`` (N,)."""
        comm = self.comm
        my_y = test_data['y']
        if isinstance(my_y, DeviceArray):
            my_y = my_y.tensor
        my_N, H = my_y.shape[0], self.H
        Hprime_start, gamma_start = self.Hprime, self.gamma
        if topK == -1:
            topK = self.state_matrix.shape[0]
        dev = self.device
        buf = {'s': torch.zeros((my_N, topK, H), dtype=torch.int8, device=dev),
               'm': torch.zeros((my_N, H), dtype=torch.float64, device=dev),
               'p': torch.zeros((my_N, topK), dtype=torch.float64, device=dev),
               'gamma': torch.zeros((my_N,), dtype=torch.float64, device=dev),
               'Hprime': torch.zeros((my_N,), dtype=torch.float64, device=dev)}

        cur_y = my_y
        which = torch.ones(my_N, dtype=torch.bool, device=dev)
        try:
            while bool(which.any()):
                ind_n = torch.nonzero(which).flatten()
                logpj, cand = self.compute_lpj(anneal, model_params, {'y': cur_y})
                lp = logpj.tensor if isinstance(logpj, DeviceArray) else torch.as_tensor(np.asarray(logpj)).to(dev)
                cd = (cand.tensor if isinstance(cand, DeviceArray) else torch.as_tensor(np.asarray(cand)).to(dev)).long()
                lp = lp.contiguous() if lp.stride(1) != 1 else lp
                run_pass(lp, cd, min(topK, lp.shape[1]), ind_n, buf)
                buf['Hprime'][ind_n] = float(self.Hprime)
                buf['gamma'][ind_n] = float(self.gamma)
                if not adaptive:
                    break
                which = ((buf['s'][:, 0, :] != 0).sum(-1) == self.gamma)
                if not bool(which.any()):
                    break
                if (Hprime_max is not None and self.Hprime == Hprime_max) and \
                        (gamma_max is not None and self.gamma == gamma_max):
                    break
                cur_y = my_y[which.cpu().numpy()] if not torch.is_tensor(my_y) else my_y[which]
                print("Rank %i: For %i data points MAP state has activity equal to gamma." % (comm.rank, int(which.sum())))
                if not ((self.Hprime == self.H) or (Hprime_max is not None and self.Hprime == Hprime_max)):
                    self.Hprime += 1
                if (self.gamma == self.H) or (gamma_max is not None and self.gamma == gamma_max):
                    continue
                self.gamma += 1
                print("Rank %i: Updating state matrix and running again." % comm.rank)
                regenerate()
        finally:
            self.Hprime, self.gamma = Hprime_start, gamma_start
            restore()
        return buf

    @staticmethod
    def _refuse_nan(top_idx):
        """Fewer than topK comparable log-joints in some row (NaN: a non-finite datapoint or parameter).  The reference's
        argsort would rank the NaNs somewhere and carry on; indexing with -1 here would silently report a wrapped state --
        refuse instead."""
        if bool((top_idx < 0).any()):
            raise _lib.HipError("inference: non-finite log-joints (NaN) in %d datapoint(s)"
                                % int((top_idx < 0).any(dim=1).sum()))

    @staticmethod
    def _inference_result(buf, logprob):
        m_out = buf['m'] if logprob else torch.exp(buf['m'])
        return {'s': buf['s'].cpu().numpy(), 'm': m_out.cpu().numpy(), 'p': buf['p'].cpu().numpy(),
                'gamma': buf['gamma'].cpu().numpy(), 'Hprime': buf['Hprime'].cpu().numpy()}

    def inference(self, anneal, model_params, test_data, topK=10, logprob=False, adaptive=True,
                  Hprime_max=None, gamma_max=None, exact=False):
        """Top-K posterior states and marginals per datapoint (camodels/__init__.py:256-375).

        Same return dict as the reference: ``s`` (N,topK,H) int8, ``m`` (N,H), ``p`` (N,topK),
        ``gamma`` / ``Hprime`` (N,).  With ``adaptive`` the datapoints whose MAP state has exactly
        gamma active units are re-run with Hprime+1 / gamma+1 (the state table is regenerated) until
        none remain or the caps are reached.  The log-joints come from the HIP E-step; the
        normalisation, top-K and marginals run on the device too.

        ``exact=True`` (BSC, MCA, MMCA): the same dict over the model's WHOLE state space {0,1}^H by
        enumeration on the device (pm_infer_exact_*), for the model and parameters of ``log_likelihood(exact=True)`` (T = 1):
        no candidates, no state table, nothing truncated.  ``s``: the topK states of largest log-joint, best first; of two
        states with equal log-joints the one with the smaller state index sum_h s_h 2^h comes first (a function of (value,
        index) alone, unlike the reference's argsort).  ``p``: with ``logprob`` the normalised log posterior l_n(s) - v_n, v_n
        the log-sum-exp over all 2^H states; without it exp(l_n(s) - l_n(s_best)) as in the truncated call (column 0 is 1).
        ``m``: P(s_h = 1 | y_n) over all states -- the bits of ``encode(exact=True)[1]`` -- or its log.  ``gamma`` and
        ``Hprime`` hold H.  With topK above 2^H the first 2^H entries of ``s`` and ``p`` are written and the rest stay zero.
        ``adaptive`` has nothing to act on and is ignored.  A row's results depend on that row and the parameters alone: the
        same bits from both libraries, under a row permutation, in a shard and on a second call; the training state is left
        as it was.  Refused before any launch: ``NotImplementedError`` for DSC, TSC and GSC, for ``anneal['T'] != 1`` and for
        a ``'mask'`` or ``'weight'`` in ``test_data``; ``ValueError`` for ``Hprime_max`` / ``gamma_max`` (nothing to grow) and
        for topK = -1, topK < 1 or topK > 16 (``EXACT_MAX_TOPK``, the length of a thread's list in the kernel); ``HipError``
        past the limits of ``reconstruct(exact=True)`` (H > 32; MCA / MMCA D > 1024).  A NaN log-joint raises ``HipError``
        as in the truncated call."""
        if exact:
            return self._inference_exact(anneal, model_params, test_data, topK, logprob, Hprime_max, gamma_max)
        from . import generate_state_matrix
        assert 'y' in test_data, "Key 'y' in test_data dict not defined."
        model_params = self.check_params(model_params)
        H, dev = self.H, self.device

        def run_pass(lp, cd, k_eff, ind_n, buf):
            n_cur, Hp = lp.shape[0], self.Hprime
            # top-K columns of the normalised posterior and the log-marginals: one HIP pass over the rows
            # (csrc/infer_kernels.hip).  Upstream quirk (:309-312): logprob=False reports exp(logpj - max), NOT the
            # normalised value -- the kernel returns both
            SMh = self.state_matrix.astype(np.int64)
            mk = (SMh << np.arange(SMh.shape[1])[None, :]).sum(axis=1).astype(np.uint16) if SMh.size else np.zeros(1, np.uint16)
            masks_d = torch.from_numpy(mk.view(np.int16).copy()).to(dev)
            cd32 = cd.to(torch.int32).contiguous()
            top_idx32 = torch.empty((n_cur, k_eff), dtype=torch.int32, device=dev)
            top_val = torch.empty((n_cur, k_eff), dtype=torch.float64, device=dev)
            top_rel = torch.empty((n_cur, k_eff), dtype=torch.float64, device=dev)
            m_blk = torch.empty((n_cur, H), dtype=torch.float64, device=dev)
            self._call("infer_topk", "pm_infer_topk_f64", _ptr(lp), lp.stride(0), _ptr(cd32), _ptr(masks_d), n_cur, H, Hp,
                       self.no_states, k_eff, _ptr(top_idx32), _ptr(top_val), _ptr(top_rel), _ptr(m_blk), H, self._stream())
            self._refuse_nan(top_idx32)
            top_idx = top_idx32.long()
            # top-K states as H-dimensional binary vectors
            SM = torch.from_numpy(self.state_matrix.astype(np.int8)).to(dev) if self.no_states else \
                torch.zeros((1, Hp), dtype=torch.int8, device=dev)
            # upstream quirk (:313-319): a re-run datapoint's earlier entries are never cleared -- one-cause
            # states only SET their bit, the null state writes nothing, multi-cause states overwrite the
            # candidate positions; start from what is there
            s_blk = buf['s'][ind_n, :k_eff].clone()
            single = (top_idx >= 1) & (top_idx <= H)
            if bool(single.any()):
                nn_, mm_ = torch.nonzero(single, as_tuple=True)
                s_blk[nn_, mm_, top_idx[nn_, mm_] - 1] = 1
            multi = top_idx > H
            if bool(multi.any()):
                nn_, mm_ = torch.nonzero(multi, as_tuple=True)
                rows = SM[top_idx[nn_, mm_] - H - 1]                           # (M, Hp)
                s_blk[nn_[:, None].expand(-1, Hp), mm_[:, None].expand(-1, Hp), cd[nn_]] = rows
            buf['s'][ind_n, :k_eff] = s_blk
            buf['p'][ind_n, :k_eff] = top_val if logprob else torch.exp(top_rel)
            buf['m'][ind_n] = m_blk        # log p(s_h = 1 | y): log-sum-exp over the states containing h (the kernel)

        def regenerate():
            (self.state_list, self.no_states, self.state_matrix,
             self.state_abs) = generate_state_matrix(self.Hprime, self.gamma)

        def restore():
            self.comm.Barrier()
            regenerate()

        return self._inference_result(self._adaptive_inference(anneal, model_params, test_data, topK, adaptive, Hprime_max,
                                                               gamma_max, run_pass, regenerate, restore), logprob)

    # ---- exact inference ------------------------------------------------------------------------------------
    EXACT_MAX_TOPK = 16               # PM_INFER_EXACT_MAX_TOPK: the entries a thread of the enumeration kernel keeps

    def _inference_exact_admit(self, anneal, model_params, test_data, topK, Hprime_max, gamma_max):
        """Everything that refuses ``inference(exact=True)``, before anything reaches the device: the model, the annealing
        point, the caps, topK, a mask or weight, and the kernels' limits (from pm_infer_exact_plan, which needs no device).
        Returns topK as an int."""
        name = type(self).__name__
        if not self._binary_latents:
            raise NotImplementedError("%s.inference: exact=True is not built for this model (the reference defines the "
                                      "marginals of DSC, TSC and GSC on the truncated table); BSC_ET, MCA_ET and MMCA_ET "
                                      "have it" % name)
        if float(anneal['T']) != 1.0:
            raise NotImplementedError("%s.inference: exact=True is the T = 1 model, got T = %r" % (name, anneal['T']))
        if Hprime_max is not None or gamma_max is not None:
            raise ValueError("%s.inference: exact=True with Hprime_max / gamma_max: nothing is truncated, so there is "
                             "nothing to grow" % name)
        if topK != int(topK) or topK < 1 or topK > self.EXACT_MAX_TOPK:
            raise ValueError("%s.inference: exact=True needs 1 <= topK <= %d (the length of a thread's list in the "
                             "enumeration kernel; topK = -1 is not built), got %r" % (name, self.EXACT_MAX_TOPK, topK))
        for key in ('mask', 'weight'):
            if test_data.get(key) is not None:
                raise NotImplementedError("%s.inference: exact=True with a %s is not built (the enumeration kernels "
                                          "read every dimension)" % (name, key))
        kind, arrays, _ = self._loglik_exact(dict(model_params))
        K = int(arrays["values"].shape[0]) if kind == "lin" else 0
        plan = (ctypes.c_int64 * 12)()
        rc = _lib.load(self.deterministic).pm_infer_exact_plan({"lin": 0, "mca": 1}[kind], 0, self.D, K, self.H, int(topK),
                                                               plan)
        if rc:
            raise _lib.HipError("%s.inference: exact=True holds H <= 32 latents%s (pm_infer_exact_%s_f64 returned %d), got "
                                "H = %d, D = %d" % (name, " and D <= 1024" if kind == "mca" else "", kind, rc, self.H, self.D))
        return int(topK)

    def _inference_exact(self, anneal, model_params, test_data, topK, logprob, Hprime_max, gamma_max):
        """``inference(exact=True)``: state indices, log-joints and v_n by pm_infer_exact_lin_f64 (BSC) or
        pm_infer_exact_mca_f64 (MCA / MMCA) from the ``_loglik_exact`` hook, the states decoded from their indices on the
        device, the marginals from ``_encode_exact``; one download, of the dict's arrays."""
        assert 'y' in test_data, "Key 'y' in test_data dict not defined."
        topK = self._inference_exact_admit(anneal, model_params, test_data, topK, Hprime_max, gamma_max)
        y, H = test_data['y'], self.H
        N = int(y.shape[0])
        if N == 0:
            return {'s': np.zeros((0, topK, H), dtype=np.int8), 'm': np.zeros((0, H)), 'p': np.zeros((0, topK)),
                    'gamma': np.zeros(0), 'Hprime': np.zeros(0)}
        with self._evaluation():
            dev = self.device
            _, _, entry = self._exact_entry(dict(model_params), "infer")
            Y = self._resident(y)["Y"]
            D = Y.shape[1]
            cols = min(topK, 1 << H)
            top_idx = torch.empty((N, cols), dtype=torch.int64, device=dev)
            top_l = torch.empty((N, cols), dtype=torch.float64, device=dev)
            v = torch.empty(N, dtype=torch.float64, device=dev)
            lib = _lib.load(self.deterministic)
            work = torch.empty(max(int(lib.pm_infer_exact_work_len(N, H, topK)), 1), dtype=torch.float64, device=dev)
            entry(lambda name, *a: self._call("infer_exact", name, *a), _ptr(Y), max(int(Y.stride(0)), D), N, topK,
                  _ptr(top_idx), cols, _ptr(top_l), cols, _ptr(v), _ptr(work))
            self._refuse_nan(top_idx)
            s = torch.zeros((N, topK, H), dtype=torch.int8, device=dev)
            s[:, :cols] = ((top_idx[:, :, None] >> torch.arange(H, device=dev)) & 1).to(torch.int8)
            p = torch.zeros((N, topK), dtype=torch.float64, device=dev)
            p[:, :cols] = (top_l - v[:, None]) if logprob else torch.exp(top_l - top_l[:, :1])
            prob = self._encode_exact(dict(model_params), y, N)[1]
            m = torch.log(prob) if logprob else prob
            full = np.full(N, float(H))
            return {'s': s.cpu().numpy(), 'm': m.cpu().numpy(), 'p': p.cpu().numpy(), 'gamma': full, 'Hprime': full.copy()}

    # ---- held-out log-likelihood --------------------------------------------------------------------------
    # What a log_likelihood call swaps out: the resident shard, the parameter products computed on it, the workspaces and
    # the pinned staging buffers live in an evaluation slot of their own; the records the last M-step left for the next
    # training step (seeded products, a speculative E-step pass, ranked candidates, next power tables) are hidden from it.
    _EVAL_SLOT = ("_data", "_par", "_ws", "_pin", "_pin_out")
    _EVAL_HIDDEN = ("_seed_rec", "_seed", "_spec", "_spec_estep", "_sel_seed", "_next_tabs", "_mstep_res", "_a0", "_nz")

    def _eval_begin(self):
        saved = dict(self.__dict__)
        slot = saved.get("_eval_slot") or {k: {} for k in self._EVAL_SLOT}
        for k in self._EVAL_SLOT:
            setattr(self, k, slot[k])
        for k in self._EVAL_HIDDEN:
            if k in saved:
                setattr(self, k, None)
        self._in_step = False
        self._loglik_eval = True         # (E-steps skip the M-step statistics they could fuse: nobody reads them)
        return saved

    def _eval_end(self, saved):
        slot = {k: self.__dict__[k] for k in self._EVAL_SLOT}
        gen = self.__dict__.get("_data_gen", 0)
        self.__dict__.clear()
        self.__dict__.update(saved)      # every attribute as the training loop left it
        self._eval_slot = slot
        self._data_gen = gen             # (shard keys stay unique across both slots)

    @contextlib.contextmanager
    def _evaluation(self, rows_gemm=True):
        """The scope every read-out runs in: ``_eval_begin`` / ``_eval_end`` around the body."""
        saved = self._eval_begin()
        try:
            if rows_gemm:
                # every product of the pass through the one-kernel GEMM, on parameter products of its own: a row of the result
                # is a function of that row of the data and of the parameters alone (attributes of the evaluation only).
                # ``log_likelihood`` without a mask or weight (plain and exact) passes False on purpose: it scores the data
                # with the training step's own products, as it did before these attributes existed, and its bits stay those.
                self._par, self._rows_gemm = {}, True
            yield
        finally:
            if rows_gemm:
                self._par = {}
            self._eval_end(saved)

    def _f64_dev(self, x):
        """``x`` as a C-contiguous float64 tensor on the device."""
        return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(self.device)

    def _mu_dev(self, mu):
        """The (D,) device copy of a mean, None for None."""
        return None if mu is None else self._f64_dev(mu).reshape(-1)

    @staticmethod
    def _nonzero_mu(mu):
        """``mu``, or None for a mean that is absent or all zeros (the kernels then skip it)."""
        return mu if mu is not None and np.any(np.asarray(mu)) else None

    @staticmethod
    def _row_stride(X, K):
        """Leading dimension of the (N, K) rows of ``X``: a single row may carry any stride, so at least K."""
        N = X.shape[0]
        return X.stride(0) if N > 1 else max(int(X.stride(0)), K)

    def _loglik_terms(self, model_params, my_data):
        """Per model: ``(logpj, a, c)`` -- the (N, K) device log-joints of the T = 1 E-step over exactly the states it scores
        for each datapoint (any row stride), the scale a of the row log-sum-exp and the per-datapoint constant c(Theta) the
        log-joints leave out, so that log sum_s p(s, y_n | Theta) = log sum_s exp(a logpj[n, s]) + c."""
        raise NotImplementedError("%s has no log_likelihood" % type(self).__name__)

    def _loglik_exact(self, model_params):
        """Per model: what ``log_likelihood(..., exact=True)`` hands the enumeration kernels (include/prosper_hip.h,
        pm_loglik_exact_*): ``(kind, arrays, scalars)`` with kind 'lin' (BSC, TSC, DSC), 'mca' (MCA, MMCA) or 'gsc'.  Host
        products of the parameters only; the data never leaves the device."""
        raise NotImplementedError("%s has no exact log_likelihood" % type(self).__name__)

    def _exact_linear(self, W, sigma, values, logp, mu=None):
        """The 'lin' hook of ``_loglik_exact`` for y ~ N(mu + W s, sigma^2 I): P = W / sigma^2, G = W^T W / sigma^2, the
        per-latent log-prior table ``logp`` (H, K) over ``values`` (K,)."""
        W = np.asarray(W, dtype=np.float64)
        s2 = float(sigma) ** 2
        arrays = {"P": W / s2, "G": (W.T @ W) / s2, "logp": np.asarray(logp, dtype=np.float64),
                  "values": np.asarray(values, dtype=np.float64)}
        if mu is not None:
            arrays["mu"] = np.asarray(mu, dtype=np.float64).reshape(-1)
        return "lin", arrays, {"cst": -0.5 * self.D * np.log(2 * np.pi * s2), "qcoef": -0.5 / s2}

    def _loglik_estep(self, model_params, my_data):
        """select_Hprimes + E_step at ``LoglikPoint`` through the training kernels: the (N, K) device log-joints."""
        data = self.select_Hprimes(model_params, my_data)
        return self.E_step(LoglikPoint(), model_params, data)['logpj'].tensor

    def log_likelihood(self, model_params, my_data, per_datapoint=False, exact=False):
        """Held-out log-likelihood F(Theta; Y) = sum_n log sum_{s in K_n} p(s, y_n | Theta) of ``my_data['y']`` (host
        array, torch tensor or DeviceArray) under ``model_params``.

        K_n is exactly the state set the model's E-step scores for y_n (the columns of its ``logpj``), p the model's full
        generative joint (prior over all H units, no A_pi_gamma renormalisation), evaluated at T = 1 with no prior
        annealing, data truncation, partial data or parameter noise.  Where K_n holds distinct states of the model, F is a
        lower bound on log p(Y | Theta), exact when K_n holds every state (H' = gamma = H).  TSC is the exception: its
        candidates may repeat a latent (tsc_et.py:142-213), and then K_n holds pseudo-states (a latent counted at two
        positions) and neither the bound nor exactness holds for that row.  Each model's ``_loglik_terms`` derives its constant c(Theta).

        Returns the sum over ALL ranks' datapoints as a float (a collective call: the per-rank sums are added in rank
        order, so every rank returns the same bits), or with ``per_datapoint=True`` this rank's (my_N,) float64 values in
        datapoint order (no collective).  ``model_params``, the training shard's residency, the records the last M-step
        left for the next step and Hprime / gamma are left as they were: a call between two EM steps does not change the
        training trajectory.  Runs the E-step kernels and pm_rows_lse_f64 on the device.

        ``exact=True``: log p(y_n | Theta) = log sum_{all s} p(s, y_n | Theta) summed over the model's WHOLE state space by
        enumeration on the device (pm_loglik_exact_*), the same generative model at the same annealing point:
        no candidates, no state table, no E-step, and a result independent of Hprime, gamma and the annealing state.  The
        state count is bounded (include/prosper_hip.h): past the bound this raises ``HipError``.

        ``my_data['mask']`` (N, D; non-zero = observed; BSC, MCA and MMCA): log sum_{s in K_n} p(s, y_obs,n), the
        unobserved dimensions left out of the likelihood and never read into the arithmetic.  Other models and
        ``exact=True`` raise ``NotImplementedError``, a mask of another shape ``ValueError``.

        ``my_data['weight']`` (N, D; finite and >= 0; BSC, MCA and MMCA): entry (n, d) was observed with noise
        variance sigma^2 / weight[n, d], 0 = not observed -- log sum_{s in K_n} p(s, y_n | weight_n), including the term 1/2
        sum_{weight > 0} log weight.  The refusals are those ``reconstruct`` documents."""
        if my_data.get('mask') is not None or my_data.get('weight') is not None:
            return self._log_likelihood_masked(model_params, my_data, per_datapoint, exact)
        if exact:
            return self._log_likelihood_exact(model_params, my_data, per_datapoint)
        with self._evaluation(rows_gemm=False):
            logpj, a, c = self._loglik_terms(dict(model_params), {'y': my_data['y']})
            rows, total = self._rows_lse(logpj, a, per_datapoint)
            if per_datapoint:
                return rows.cpu().numpy() + c
            local = float(total.cpu()[0]) + logpj.shape[0] * c
        return self._sum_over_ranks(local)

    def _rows_lse(self, logpj, a, per_datapoint):
        """pm_rows_lse_f64 on the (N, K) log-joints: (rows (N,) or None, total (1,)) of log sum_k exp(a logpj[n, k])."""
        N, K = logpj.shape
        lib = _lib.load(self.deterministic)
        work = torch.empty(int(lib.pm_rows_lse_work_len(N)), dtype=torch.float64, device=self.device)
        total = torch.empty(1, dtype=torch.float64, device=self.device)
        rows = torch.empty(N, dtype=torch.float64, device=self.device) if per_datapoint else None
        self._call("loglik_rows", "pm_rows_lse_f64", _ptr(logpj), self._row_stride(logpj, K), N, K, ctypes.c_double(a), None,
                   _ptr(rows), _ptr(work), _ptr(total), self._stream())
        return rows, total

    def _sum_over_ranks(self, local):
        """The ranks' values added in rank order: every rank returns the same bits."""
        out = 0.0
        for v in self.comm.allgather(local):
            out += v
        return out

    # ---- posterior-mean reconstruction --------------------------------------------------------------------
    _recon_var_max_D = 2 ** 30        # (MCA / MMCA: 1024, the lanes-over-dimensions kernels)

    def _recon_layout(self, model_params):
        """Per model: what ``reconstruct`` needs beside the E-step's log-joints -- ``params`` (the parameters the E-step is
        run with), ``blocks`` (the latent value of every block of H one-cause columns, starting at column ``soff``),
        ``table`` ((S, Hprime) latent values per candidate position of the table states, starting at column ``moff``; None:
        no table term in E[s]), ``W`` (D, H) and ``mu`` (D,) or None of the mean ybar(s) = mu + W s; ``mca``: True when the
        multi-cause states' mean is the rho-combination instead (pm_recon_mca_f64)."""
        raise NotImplementedError("%s has no reconstruct" % type(self).__name__)

    def _layout_dev(self, table, blocks):
        """A state layout as the kernels take it: (S, the (S, Hprime) table on the device or None, the 8-double vector of
        ``blocks``)."""
        S = 0 if table is None else int(table.shape[0])
        bv = (ctypes.c_double * 8)(*([float(v) for v in blocks] + [0.0] * (8 - len(blocks))))
        return S, (self._f64_dev(table) if S else None), bv

    def _layout_call(self, label, entry, lp, cand, lay, table, *out):
        """pm_recon_expect_f64, pm_recon_moments2_f64 or pm_encode_f64: the arguments they share -- the log-joints ``lp`` with
        their own log-sum-exp, scale 1 and no offsets, the candidates and the layout ``lay`` with ``table`` --, then ``out``."""
        N, K = lp.shape
        S, tab_d, bv = self._layout_dev(table, lay["blocks"])
        self._call(label, entry, _ptr(lp), self._row_stride(lp, K), None, ctypes.c_double(1.0), None, _ptr(cand) if S else None,
                   _ptr(tab_d), bv, N, self.H, self.Hprime if S else 0, K, lay["soff"], len(lay["blocks"]), lay["moff"], S,
                   *out, self._stream())

    def _recon_expect(self, lp, cand, lay, ones=False):
        """pm_recon_expect_f64 into an (N, Kp) workspace, Kp = H (+ 1 for the column of ones) padded to a multiple of 8 with
        zero columns: the K range of the product that follows."""
        H = self.H
        Kp = (H + (1 if ones else 0) + 7) // 8 * 8
        es = self._buf("recon_es", (lp.shape[0], Kp))
        self._layout_call("recon_expect", "pm_recon_expect_f64", lp, cand, lay, lay.get("table"), _ptr(es), Kp, Kp,
                          H if ones else -1)
        return es

    def _recon_product(self, es, W, mu=None):
        """Yhat (N, D) = es . [W | mu | 0]^T through pm_gemm_nt_rows_f64 (``es`` carries a column of ones at H when ``mu`` is
        given)."""
        (N, cols), D, H = es.shape, self.D, self.H
        Wp = np.zeros((D, cols))
        Wp[:, :H] = np.asarray(W, dtype=np.float64)
        if mu is not None:
            Wp[:, H] = np.asarray(mu, dtype=np.float64).reshape(-1)
        Wd = torch.from_numpy(Wp).to(self.device)
        out = torch.empty((N, D), dtype=torch.float64, device=self.device)
        self._call("recon_gemm", "pm_gemm_nt_rows_f64", _ptr(es), cols, _ptr(Wd), cols, _ptr(out), D, N, D, cols,
                   self._stream())
        return out

    def _recon_variance(self, lp, cand, lay, Yhat, mu, par=None):
        """The (N, D) device tensor V of ``reconstruct(variance=True)`` from the log-joints, candidates and
        layout ``Yhat`` was formed from: m2 and p by pm_recon_moments2_f64, sum_h m2 W_dh^2 as one pm_gemm_nt_rows_f64
        against W o W, MCA / MMCA's multi-cause squares by pm_recon_mca_var_f64, then pm_recon_var_finish_f64."""
        H, Hp, N = self.H, self.Hprime, lp.shape[0]
        table = lay.get("table")
        npair = Hp * (Hp - 1) // 2 if table is not None and table.shape[0] else 0
        Kp = (H + 7) // 8 * 8
        m2 = self._buf("recon_m2", (N, Kp))
        p2 = self._buf("recon_p2", (N, npair)) if npair else None
        self._layout_call("recon_var", "pm_recon_moments2_f64", lp, cand, lay, table, _ptr(m2), Kp, Kp, _ptr(p2),
                          max(npair, 1))
        mca = None
        if lay.get("mca") and self.no_states:
            mca = lambda V: self._recon_mca("recon_var", "pm_recon_mca_var_f64", lp, cand, par, V)
        return self._recon_var_product(m2, p2, cand, lay["W"], mu, Yhat, more=mca)

    def _recon_mca(self, label, entry, lp, cand, par, out):
        """pm_recon_mca_f64 / pm_recon_mca_var_f64: the multi-cause states' rho-combinations (their squares) added to ``out``."""
        N, K = lp.shape
        self._call(label, entry, _ptr(lp), self._row_stride(lp, K), None, _ptr(cand), _ptr(self._masks()), _ptr(par["Wrho"]),
                   ctypes.c_double(1. / par["rho"]), int(bool(self.signed_w)), N, self.H, self.D, self.Hprime, self.no_states,
                   _ptr(out), self.D, self._stream())

    def _recon_var_product(self, m2, p2, cand, W, mu, Yhat, more=None):
        """V (N, D) from the second moments: sum_h m2 W_dh^2 as one pm_gemm_nt_rows_f64 of ``m2`` (N, Kp; zero past H) against
        W o W, ``more(V)`` (MCA / MMCA: the multi-cause squares), then pm_recon_var_finish_f64 with the pairs ``p2`` (N,
        H'(H'-1)/2; None: no pair term) over ``cand``, ``Yhat`` and ``mu`` (None: 0)."""
        N, Kp = m2.shape
        H, D, Hp = self.H, self.D, self.Hprime
        npair = 0 if p2 is None else int(p2.shape[1])
        W = np.asarray(W, dtype=np.float64)
        W2 = np.zeros((D, Kp))
        W2[:, :H] = W * W
        W2d = torch.from_numpy(W2).to(self.device)
        V = torch.empty((N, D), dtype=torch.float64, device=self.device)
        self._call("recon_var", "pm_gemm_nt_rows_f64", _ptr(m2), Kp, _ptr(W2d), Kp, _ptr(V), D, N, D, Kp, self._stream())
        if more is not None:
            more(V)
        Wt = self._f64_dev(W.T) if npair else None
        mu_d = self._mu_dev(mu)
        self._call("recon_var", "pm_recon_var_finish_f64", _ptr(V), D, _ptr(Yhat), D, _ptr(mu_d), _ptr(p2), max(npair, 1),
                   _ptr(cand) if npair else None, _ptr(Wt), D, N, H, D, Hp if npair else 0, self._stream())
        return V

    def _logjoints(self, model_params, y, obs):
        """What every read-out consumes, in the dict of ``_obs_estep``: ``logpj`` (N, K) and ``cand`` (N, Hprime), the device
        log-joints and candidates of the selection and T = 1 E-step, and ``lay`` (``_recon_layout``) -- from the model's
        ``_obs_estep`` when ``obs`` (what ``_observation`` returned) is given, which keeps the plain layout and for MCA adds
        ``par``, else from the plain selection and E-step.  The caller holds the dict, and with it every tensor of the E-step,
        for as long as it works on them."""
        if obs is not None:
            return self._obs_estep(model_params, y, obs)
        lay = self._recon_layout(model_params)
        mp = lay["params"]
        data = self.select_Hprimes(mp, {'y': y})
        lp = self.E_step(LoglikPoint(), mp, data)['logpj'].tensor
        return {"logpj": lp, "cand": self._device_candidates(data['candidates'], lp.shape[0]), "lay": lay}

    def _mca_tables(self, out, y):
        """MCA / MMCA's power tables at T = 1: those ``_logjoints`` handed out, or the ones its plain E-step built."""
        par = out.get("par")
        return par if par is not None else self._tables_for(out["lay"]["params"]['W'], 1.0, self._resident(y))

    def _reconstruct(self, model_params, y, obs, N, variance=False):
        """The (N, D) device tensor of ``reconstruct`` for the models whose E-step leaves (N, K) log-joints (``obs``: None or
        what ``_observation`` returned -- the expectation and product kernels are the same, so the estimate covers all D
        dimensions); with ``variance`` the pair (Yhat, V)."""
        out = self._logjoints(model_params, y, obs)
        lp, cand, lay, par = out["logpj"], out["cand"], out["lay"], out.get("par")
        # (the rows' log-sum-exp is formed again by the kernels, not taken from the E-step: the fused E-step kernels reduce a
        # row in an order that depends on the tile shape its position in the shard gets, so their ``lse`` differs in the last
        # bit between a row of a whole array and the same row of a shard -- and a row of Yhat must not)
        mu = self._nonzero_mu(lay.get("mu"))
        Yhat = self._recon_product(self._recon_expect(lp, cand, lay, ones=mu is not None), lay["W"], mu)
        if lay.get("mca") and self.no_states:
            par = self._mca_tables(out, y)
            self._recon_mca("recon_mca", "pm_recon_mca_f64", lp, cand, par, Yhat)
        if variance:
            return Yhat, self._recon_variance(lp, cand, lay, Yhat, mu, par)
        return Yhat

    def reconstruct(self, model_params, my_data, device=False, exact=False, variance=False):
        """Posterior-mean denoising: yhat_n = sum_{s in K_n} q_n(s) ybar(s; Theta), q_n(s) = p(s, y_n | Theta) / sum_{s' in K_n}
        p(s', y_n | Theta), for ``my_data['y']`` (host array, torch tensor or DeviceArray): the model's estimate of the
        noiseless data.  K_n and p are exactly those of ``log_likelihood``: the state set the E-step scores
        for y_n, the full generative joint, at T = 1 with no prior annealing, data truncation, partial data or parameter
        noise; ybar(s) is the mean of the data given the state (mu + W s for the linear models, the
        rho-combination the E-step evaluates for MCA / MMCA, W_s E[z_s | s, y_n] for GSC).  No weight is dropped or
        thresholded.  At H' = gamma = H this is the exact posterior mean, the minimum-mean-square estimate.  TSC's candidates
        may repeat a latent (tsc_et.py:142-213): such a row holds pseudo-states, whose mean counts the latent at both
        positions, as the E-step's energy does; the exactness does not hold for that row.

        Returns this rank's (my_N, D) float64 rows in datapoint order as a NumPy array, or with ``device=True`` as a
        ``DeviceArray`` left on the device; there is no collective.  A NaN in a data row makes that row NaN and no other.
        ``model_params``, the training shard's residency, the records the last M-step left and Hprime / gamma stay as they
        were: a call between two EM steps does not change the training trajectory.  The results do not depend on
        ``deterministic``.  Runs the E-step kernels, pm_recon_* and pm_gemm_nt_rows_f64 on the device.

        ``my_data['mask']`` (N, D; non-zero = observed; NumPy, torch or DeviceArray of any numeric type; BSC,
        MCA and MMCA): q_n comes from the joint of the observed dimensions alone, yhat_n still covers all D -- the missing
        ones are inpainted.  Whatever an unobserved entry holds changes no bit; a row's bits depend on that row of ``y``,
        that row of the mask and the parameters alone.  Other models raise ``NotImplementedError`` before any launch.

        ``my_data['weight']`` (N, D; NumPy, torch or DeviceArray of any real numeric type -- a float64 device tensor with unit
        column stride is used in place; BSC, MCA and MMCA): entry (n, d) was observed with noise variance sigma^2 /
        weight[n, d], 0 = not observed; a mask is the weight restricted to {0, 1} and such a weight returns the masked call's
        bits.  Whatever ``y`` holds at weight 0 changes no bit.  Raised before any launch: ``ValueError`` for a weight that is
        negative, NaN or infinite anywhere (one reduction where the weight lives), of another shape, or given together with
        ``'mask'`` (fold the mask into the weight as zeros); ``NotImplementedError`` for ``exact=True`` and for the other
        models; ``HipError`` for H' > 16.

        ``exact=True``: yhat_n = sum_{all s} p(s | y_n, Theta) ybar(s) over the model's WHOLE state space by enumeration on
        the device (pm_recon_exact_*), the same generative model, parameters and ybar(s): no candidates, no
        state table, no E-step, and a result independent of Hprime, gamma and the annealing state.  A row's bits depend on
        that row of ``y`` and the parameters alone.  The state count is bounded as for ``log_likelihood(exact=True)`` (MCA /
        MMCA also D <= 1024): past the bound this raises ``HipError``.  Together with ``my_data['mask']`` it raises
        ``NotImplementedError``.

        ``variance=True``: returns ``(Yhat, V)``, both NumPy arrays or both ``DeviceArray``, V_nd = E_q[(ybar_d(s) -
        yhat_nd)^2] = E_q[ybar_d^2] - yhat_nd^2 under the same q_n over the same K_n (GSC: over z | s, y_n too): the posterior
        variance of the NOISELESS value -- the predictive variance of a new observation is V + sigma^2 (GSC: + Sigma_dd), which
        the caller adds.  ``Yhat`` has the bits of the call without the keyword.  At H' = gamma = H it is the exact posterior
        variance; with ``my_data['mask']`` the variance given the observed dimensions, at every dimension.  A value rounding
        takes below 0 is returned as 0; a NaN data row gives a NaN row of V and touches no other.  Together with
        ``exact=True`` it raises ``NotImplementedError`` before any launch (the enumeration kernels keep no second
        moments).  Runs pm_recon_moments2_f64, pm_recon_mca_var_f64, pm_recon_var_finish_f64 and one more
        pm_gemm_nt_rows_f64."""
        y = my_data['y']
        N = int(y.shape[0])
        obs = self._observation(my_data)
        if obs is not None:
            self._masked_admit(y, obs[1], exact, what="reconstruct", key=obs[0])
        if variance and exact:
            raise NotImplementedError("%s.reconstruct: variance=True with exact=True is not built (the enumeration kernels "
                                      "keep no second moments)" % type(self).__name__)
        if variance and self.Hprime > 16:
            raise _lib.HipError("%s.reconstruct: variance=True holds H' <= 16 candidates, got %d"
                                % (type(self).__name__, self.Hprime))
        if variance and self.D > self._recon_var_max_D:
            raise _lib.HipError("%s.reconstruct: variance=True holds D <= %d (pm_recon_mca_var_f64), got %d"
                                % (type(self).__name__, self._recon_var_max_D, self.D))
        if N == 0:
            empty = lambda: DeviceArray(torch.empty((0, self.D), dtype=torch.float64, device=self.device)) if device \
                else np.empty((0, self.D))
            return (empty(), empty()) if variance else empty()
        with self._evaluation():
            if exact:
                Yhat = self._reconstruct_exact(dict(model_params), y, N)
            else:
                Yhat = self._reconstruct(dict(model_params), y, obs, N, variance)
            if variance:
                return tuple(DeviceArray(t) if device else t.cpu().numpy() for t in Yhat)
            return DeviceArray(Yhat) if device else Yhat.cpu().numpy()

    # ---- latent codes -------------------------------------------------------------------------------------
    _binary_latents = False           # BSC, MCA, MMCA: s_h in {0, 1} -- prob is min(mean, 1), and ``encode(exact=True)`` is built

    def _encode_from(self, lp, N, cand, lay):
        """(mean, prob), two (N, H) device tensors, by pm_encode_f64 from the log-joints ``lp``, the candidates and the layout
        (``_recon_layout``) that ``reconstruct`` reads; ``lay['encode_table']`` is the table of a model whose reconstruction
        needs none (MCA / MMCA)."""
        H = self.H
        mean = torch.empty((N, H), dtype=torch.float64, device=self.device)
        prob = torch.empty((N, H), dtype=torch.float64, device=self.device)
        self._layout_call("encode", "pm_encode_f64", lp, cand, lay, lay.get("encode_table", lay.get("table")), _ptr(mean), H,
                          _ptr(prob), H)
        return mean, prob

    def _encode(self, model_params, y, obs, N):
        """``encode`` for the models whose E-step leaves (N, K) log-joints: the log-joints of ``_reconstruct``, then
        ``_encode_from``."""
        out = self._logjoints(model_params, y, obs)
        return self._encode_from(out["logpj"], N, out["cand"], out["lay"])

    def _encode_exact(self, model_params, y, N):
        """``encode(exact=True)`` of the binary models from the ``_loglik_exact`` hook: E[s] over all 2^H states by
        pm_recon_exact_lin_f64 (BSC) or pm_encode_exact_mca_f64 (MCA / MMCA); prob = min(E[s], 1)."""
        _, _, entry = self._exact_entry(model_params, "encode")
        self._exact_limits(entry, self.H)
        mean = self._exact_rows("encode_exact", entry, y, torch.empty((N, self.H), dtype=torch.float64, device=self.device))
        return mean, torch.clamp(mean, max=1.0)

    def _encode_admit(self, exact):
        """The refusals of ``encode`` that depend on the model alone, before any device call."""
        if exact and not self._binary_latents:
            raise NotImplementedError("%s.encode: exact=True is not built for this model (the enumeration kernels of DSC, TSC "
                                      "and GSC carry no indicator sums); BSC_ET, MCA_ET and MMCA_ET have it"
                                      % type(self).__name__)
        if not exact and self.Hprime > 16:
            raise _lib.HipError("%s.encode holds H' <= 16 candidates (pm_encode_f64), got %d"
                                % (type(self).__name__, self.Hprime))

    def encode(self, model_params, my_data, device=False, exact=False):
        """The code of every datapoint of ``my_data['y']`` (host array, torch tensor or DeviceArray): ``(mean, prob)``, both
        (my_N, H) float64 -- mean[n, h] = sum_{s in K_n} q_n(s) s_h = E[s_h | y_n] and prob[n, h] = sum_{s in K_n} q_n(s) [s_h
        != 0] = P(s_h != 0 | y_n).  K_n and q_n are exactly those of ``reconstruct`` and ``log_likelihood``: the states the
        E-step scores for y_n, weighted by the full generative joint at T = 1; no weight is dropped or thresholded.  At H' =
        gamma = H these are the exact posterior marginals.  BSC, MCA, MMCA: the latents are binary and prob = min(mean, 1).
        DSC, TSC: mean carries the latent values, prob the non-zero indicator.  A TSC row whose candidates repeat a latent
        (tsc_et.py:142-213) holds pseudo-states: mean counts the latent at both positions, as ``reconstruct`` does; prob counts
        a state once for a latent if any position holding it is non-zero, so prob <= 1 always.  GSC: mean = E[s_h z_h | y_n]
        and prob = E[s_h | y_n], the moments of the doubled-logit pass ``reconstruct`` runs (weights floored at DBL_MIN as
        there).

        Returns NumPy arrays, or with ``device=True`` two ``DeviceArray`` left on the device; there is no collective.  A NaN
        in a data row makes that row of both outputs NaN and no other.  A row's bits depend on that row (and its row of the
        mask or weight) and the parameters alone: the same from both libraries, under a row permutation, in a shard and on
        a second call.  ``model_params``, the training shard's residency, the records the last M-step left and Hprime / gamma
        stay as they were: a call between two EM steps does not change the training trajectory.  Runs the E-step kernels and
        pm_encode_f64 on the device.

        ``my_data['mask']`` / ``my_data['weight']`` (BSC, MCA and MMCA): the codes are conditioned on the
        observed entries; whatever an unobserved or zero-weight entry holds changes no bit.  The refusals are those
        ``reconstruct`` documents, raised before any launch.

        ``exact=True`` (BSC, MCA, MMCA): the marginals over the model's WHOLE state space by enumeration on the device
        (pm_recon_exact_lin_f64, pm_encode_exact_mca_f64), within the limits of ``reconstruct(exact=True)``
        (``HipError`` past them).  DSC, TSC and GSC raise ``NotImplementedError``, and so does a mask or weight with it."""
        y = my_data['y']
        N = int(y.shape[0])
        obs = self._observation(my_data)
        if obs is not None:
            self._masked_admit(y, obs[1], exact, what="encode", key=obs[0])
        self._encode_admit(exact)
        if N == 0:
            empty = lambda: DeviceArray(torch.empty((0, self.H), dtype=torch.float64, device=self.device)) if device \
                else np.empty((0, self.H))
            return empty(), empty()
        with self._evaluation():
            if exact:
                pair = self._encode_exact(dict(model_params), y, N)
            else:
                pair = self._encode(dict(model_params), y, obs, N)
            return tuple(DeviceArray(t) if device else t.cpu().numpy() for t in pair)

    # ---- posterior draws ----------------------------------------------------------------------------------
    sample_chunk_bytes = 1 << 26      # bound of the workspace beside the result (indices and active lists of one row chunk)
    sample_chunk_rows = None          # rows per chunk when set (tests): the draws do not depend on it

    @staticmethod
    def _sample_check(N, n_samples, uniforms, normals, n_normals=0):
        """The refusals of ``sample_posterior`` that need no device: ``ValueError`` for n_samples < 1, a wrongly shaped
        ``uniforms`` / ``normals`` and a host ``uniforms`` with a value outside [0, 1) or NaN.  Returns n_samples as an int."""
        M = int(n_samples)
        if M != n_samples or M < 1:
            raise ValueError("sample_posterior: n_samples must be an integer >= 1, got %r" % (n_samples,))
        for name, arr, want in (("uniforms", uniforms, (N, M)), ("normals", normals, (N, M, n_normals))):
            if arr is None:
                continue
            t = getattr(arr, "tensor", arr)
            shape = tuple(t.shape) if hasattr(t, "shape") else np.asarray(t).shape
            if name == "normals" and not n_normals:
                continue                     # (only GSC draws z: the other models ignore the argument's values)
            if shape != want:
                raise ValueError("sample_posterior: %s has shape %r, expected %r" % (name, shape, want))
        if uniforms is not None:
            t = getattr(uniforms, "tensor", uniforms)
            if not (torch is not None and torch.is_tensor(t) and t.is_cuda):
                h = t.numpy() if (torch is not None and torch.is_tensor(t)) else np.asarray(t)
                if h.size and not bool(np.all((h >= 0.0) & (h < 1.0))):
                    raise ValueError("sample_posterior: uniforms must lie in [0, 1) (a NaN or a value outside it was given)")
        return M

    def _sample_randoms(self, N, M, seed, uniforms, normals, n_normals):
        """(U (N, M), E (N, M, n_normals) or None) float64 on the device: the caller's arrays, or ``torch.rand`` and then
        ``torch.randn`` from ONE generator on the device seeded with ``seed`` (it fills the whole arrays: with ``seed`` alone a
        row's draws depend on (N, M))."""
        g = self._gen(seed) if (uniforms is None or (n_normals and normals is None)) else None

        def given(arr):
            t = getattr(arr, "tensor", arr)
            if not torch.is_tensor(t):
                t = self._f64_dev(np.asarray(t))
            return t.to(device=self.device, dtype=torch.float64).contiguous()
        U = given(uniforms) if uniforms is not None else \
            torch.rand((N, M), generator=g, device=self.device, dtype=torch.float64)
        E = None
        if n_normals:
            E = given(normals) if normals is not None else \
                torch.randn((N, M, n_normals), generator=g, device=self.device, dtype=torch.float64)
        return U, E

    _sample_n_normals = 0             # standard normals per draw (GSC: gamma, its draw of z)

    def _sample_rows(self, N, M, A):
        """Rows per chunk: idx (4 bytes) and the active list (12 A bytes) per (row, sample) within ``sample_chunk_bytes``."""
        if self.sample_chunk_rows:
            return max(1, int(self.sample_chunk_rows))
        return max(1, min(N, int(self.sample_chunk_bytes) // (M * (4 + 12 * A))))

    def _sample_states(self, X, K, n0, n, U, M):
        """pm_sample_states_f64 on rows [n0, n0 + n) of the log-joints ``X`` and of ``U``: idx (n, M) int32."""
        idx = self._buf("sample_idx", (n, M), torch.int32)
        ld = self._row_stride(X, K)
        self._call("sample_states", "pm_sample_states_f64", ctypes.c_void_p(X.data_ptr() + 8 * n0 * ld), ld, None,
                   ctypes.c_double(1.0), None, ctypes.c_double(0.0), -1,
                   ctypes.c_void_p(U.data_ptr() + 8 * n0 * M), M, n, K, M, _ptr(idx), self._stream())
        return idx

    def _sample_active(self, idx, cand_rows, n, M, K, A, layout, lay):
        """pm_sample_active_f64 with ``layout`` (what ``_layout_dev`` returned): (act_idx (n, M, A) int32, act_val (n, M, A))."""
        ai = self._buf("sample_act_idx", (n, M, A), torch.int32)
        av = self._buf("sample_act_val", (n, M, A))
        S, table_d, bv = layout
        self._call("sample_active", "pm_sample_active_f64", _ptr(idx), cand_rows if S else None, _ptr(table_d), bv, n, M, self.H,
                   self.Hprime if S else 0, K, lay["soff"], len(lay["blocks"]), lay["moff"], S, A, _ptr(ai), _ptr(av),
                   self._stream())
        return ai, av

    @staticmethod
    def _sample_scatter(idx, ai, av, H):
        """The active lists as latent values (M, n, H): a latent held by two positions (TSC) receives both values, a draw of
        -1 (a NaN row) gives NaN."""
        n, M, A = ai.shape
        ii = ai.long()
        ii = torch.where(ii < 0, torch.full_like(ii, H), ii)
        buf = torch.zeros((n, M, H + 1), dtype=torch.float64, device=ai.device)
        buf.scatter_add_(2, ii, av)
        s = buf[:, :, :H]
        s[idx < 0] = float("nan")
        return s.permute(1, 0, 2)

    def _sample(self, model_params, y, obs, N, M, U, latents, E=None):
        """The (M, N, D) device tensor of ``sample_posterior`` (and with ``latents`` the (M, N, H) one) for the models whose
        E-step leaves (N, K) log-joints: the E-step of ``reconstruct`` (``obs``: None or what ``_observation`` returned),
        then per row chunk pm_sample_states_f64, the active list and the decode kernel, written in place."""
        H, D, Hp = self.H, self.D, self.Hprime
        out = self._logjoints(model_params, y, obs)
        lp, cand, lay = out["logpj"], out["cand"], out["lay"]
        K = lp.shape[1]
        mca = bool(lay.get("mca"))
        table = lay.get("table")
        if mca:
            par = self._mca_tables(out, y)
            table = self.state_matrix if self.no_states else None
        layout = self._layout_dev(table, lay["blocks"])
        A = max(1, int((np.asarray(table) != 0).sum(axis=1).max())) if layout[0] else 1
        mu_d = self._mu_dev(self._nonzero_mu(lay.get("mu")))
        Wt = par["Wt"] if mca else self._f64_dev(np.asarray(lay["W"], dtype=np.float64).T)
        Ys = torch.empty((M, N, D), dtype=torch.float64, device=self.device)
        Sl = torch.empty((M, N, H), dtype=torch.float64, device=self.device) if latents else None
        rows = self._sample_rows(N, M, A)
        for n0 in range(0, N, rows):
            n = min(rows, N - n0)
            idx = self._sample_states(lp, K, n0, n, U, M)
            cand_rows = ctypes.c_void_p(cand.data_ptr() + 4 * n0 * Hp)
            out_p = ctypes.c_void_p(Ys.data_ptr() + 8 * n0 * D)
            if mca:
                self._call("sample_decode", "pm_sample_decode_mca_f64", _ptr(idx), cand_rows, _ptr(self._masks()), _ptr(Wt),
                           _ptr(par["Wrho"]), ctypes.c_double(1. / par["rho"]), int(bool(self.signed_w)), n, M, H, D, Hp,
                           self.no_states, out_p, D, N * D, self._stream())
            if latents or not mca:
                ai, av = self._sample_active(idx, cand_rows, n, M, K, A, layout, lay)
                if not mca:
                    self._call("sample_decode", "pm_sample_decode_lin_f64", _ptr(ai), _ptr(av), A, _ptr(Wt), D, _ptr(mu_d), n,
                               M, H, D, out_p, D, N * D, self._stream())
                if latents:
                    Sl[:, n0:n0 + n] = self._sample_scatter(idx, ai, av, H)
        return Ys, Sl

    def sample_posterior(self, model_params, my_data, n_samples=1, seed=None, latents=False, device=False, uniforms=None,
                         normals=None):
        """Posterior draws of the noiseless data: ``Ys`` (n_samples, my_N, D) float64 with Ys[m, n] = ybar(s),
        s ~ q_n(s) -- the states K_n, the weights q_n and the per-state mean ybar(s) are exactly those ``reconstruct``
        without keywords averages (mu + W s for BSC / DSC / TSC; W_h, the rho-combination at T = 1 or 0 for MCA / MMCA), so
        the mean of many draws tends to ``reconstruct``'s estimate and their variance to ``variance=True``'s.  Observation
        noise is NOT added: for a predictive draw the caller adds sigma eps, as V + sigma^2.  ``latents=True`` returns ``(Ys,
        S)``, S (n_samples, my_N, H) float64 the latent values of each draw (0 / 1, the DSC / TSC value; a TSC latent that two
        candidate positions hold carries the sum of both).  NumPy arrays, or with ``device=True`` ``DeviceArray`` handles
        left on the device; no collective.  ``model_params``, the training state and Hprime / gamma stay as they were, the
        result does not depend on ``deterministic``; the call runs in the evaluation slot.

        Randomness: U = torch.rand((my_N, n_samples)) from a ``torch.Generator`` on the device seeded with ``seed``, or the
        caller's ``uniforms`` of that shape (NumPy, torch or DeviceArray) -- then the result is a pure function of its
        inputs: a row's draws depend on that row of the data, the parameters and that row of U alone, with the same bits from
        both libraries, under a row permutation that permutes U along, in a shard and for every internal chunking.  With
        ``seed`` alone the draws depend on (my_N, n_samples): the generator fills the whole array, so a shard of the data
        does not reproduce the rows of the whole call -- pass ``uniforms`` (GSC: and ``normals``) for that.  ``normals`` is
        GSC's (its draw of z); the other models ignore it.  Draw m of row n is the smallest column k of the row's log-joints with u C < c_k, c the
        running sum of the weights in pm_sample_states_f64's order: a state of weight 0 is never drawn.

        ``my_data['mask']`` (BSC, MCA, MMCA): the draw comes from the posterior given the observed dimensions
        and covers all D -- an imputation; whatever an unobserved entry holds changes no bit.  Other models raise
        ``NotImplementedError`` before any launch.  A NaN in a data row makes that row's draws NaN and no other's.
        ``my_data['weight']``: the draw comes from the posterior under the per-entry noise variances sigma^2 /
        weight, with the refusals ``reconstruct`` documents.

        Raises ``ValueError`` for n_samples < 1, wrongly shaped ``uniforms`` / ``normals`` and host ``uniforms`` outside [0, 1),
        ``HipError`` for H' > 16 and for MCA / MMCA with D > 1024 -- all before any launch.  There is no ``exact=``.  Runs
        the E-step kernels and pm_sample_*.

        GSC: ybar = W_s z with z | s, y_n ~ N(kappa_s, Lambda_s^-1) drawn as kappa_s + L eps (pm_sample_gsc_f64), L the lower
        Cholesky factor of Lambda_s^-1 with the positions in ascending candidate order and eps the first |s| of the draw's
        gamma standard normals E[n, m, :] -- ``torch.randn((my_N, n_samples, gamma))`` from the same generator, after U, or the
        caller's ``normals`` of that shape; the state weights are the E-step's floored ones (pm_recon_gsc_moments2_f64).
        ``S`` holds s o z."""
        y = my_data['y']
        N = int(y.shape[0])
        nn = int(self._sample_n_normals)
        M = self._sample_check(N, n_samples, uniforms, normals, nn)
        obs = self._observation(my_data)
        if obs is not None:
            self._masked_admit(y, obs[1], what="sample_posterior", key=obs[0])
        if self.Hprime > 16:
            raise _lib.HipError("%s.sample_posterior holds H' <= 16 candidates, got %d" % (type(self).__name__, self.Hprime))
        if self.D > self._recon_var_max_D:
            raise _lib.HipError("%s.sample_posterior holds D <= %d (pm_sample_decode_mca_f64), got %d"
                                % (type(self).__name__, self._recon_var_max_D, self.D))
        wrap = (lambda t: DeviceArray(t)) if device else (lambda t: t.cpu().numpy())
        if N == 0:
            z = lambda c: DeviceArray(torch.empty((M, 0, c), dtype=torch.float64, device=self.device)) if device \
                else np.empty((M, 0, c))
            return (z(self.D), z(self.H)) if latents else z(self.D)
        with self._evaluation():
            U, E = self._sample_randoms(N, M, seed, uniforms, normals, nn)
            Ys, Sl = self._sample(dict(model_params), y, obs, N, M, U, latents, E)
            return (wrap(Ys), wrap(Sl)) if latents else wrap(Ys)

    # ---- missing values -----------------------------------------------------------------------------------
    _OBS_KIND = {'mask': "masked", 'weight': "weighted"}      # (the word in entry names, launch labels and messages)

    def _obs_estep(self, model_params, y, obs):
        """Per model: selection and T = 1 E-step of ``y`` under the observation record ``obs`` (what ``_observation``
        returned), run inside an evaluation with ``_rows_gemm`` set.  ``('mask', mask)``: over the dimensions the mask marks
        as observed (non-zero).  Returns a dict: ``logpj`` (N, K) device log-joints in the layout of the unmasked E-step,
        ``cand`` (N, Hprime) int32, ``dn`` (N,) int32 observed dimensions per row, ``c0`` / ``c1`` with log p(s, y_obs) = logpj
        + c0 + D_n c1, ``lay`` (``_recon_layout``), for MCA ``par`` (the power tables), and ``logw`` = None.  ``('weight',
        weight)``: ``y`` observed with the per-entry noise variances sigma^2 / weight (0 = not observed) -- the
        same dict with log p(s, y | weight) = logpj + c0 + D_n c1 + logw, ``logw`` (N,) the per-row 1/2 sum_{weight > 0} log
        weight, left on the device."""
        what = "per-entry noise weights" if obs[0] == 'weight' else "missing values"
        raise NotImplementedError("%s: %s (my_data['%s']) are not built for this model; BSC_ET, MCA_ET and MMCA_ET have the %s "
                                  "E-step" % (type(self).__name__, what, obs[0], self._OBS_KIND[obs[0]]))

    @staticmethod
    def _observation(my_data):
        """What ``my_data`` says about how its entries were observed: None, ``('mask', mask)`` or ``('weight', weight)``;
        both at once is a ``ValueError``."""
        mask, weight = my_data.get('mask'), my_data.get('weight')
        if weight is None:
            return ('mask', mask) if mask is not None else None
        if mask is not None:
            raise ValueError("my_data['weight'] together with my_data['mask']: fold the mask into the weight as zeros "
                             "(weight = 0 where mask == 0)")
        return ('weight', weight)

    def _masked_admit(self, y, mask, exact=False, what="log_likelihood", key='mask'):
        """Everything that refuses a masked (``key='mask'``) or weighted (``key='weight'``, ``mask`` the weight) call, before
        any launch: the model, ``exact=True``, the record's shape, a weight's values, H'."""
        if type(self)._obs_estep is DeviceCAModel._obs_estep:
            self._obs_estep(None, None, (key, None))
        if exact:
            raise NotImplementedError("%s.%s: exact=True with a %s is not built (the enumeration kernels "
                                      "read every dimension)" % (type(self).__name__, what, key))
        shape = tuple(getattr(mask, "tensor", mask).shape) if hasattr(getattr(mask, "tensor", mask), "shape") \
            else np.asarray(mask).shape
        if len(shape) != 2:
            raise ValueError("my_data['%s'] must be two-dimensional (N, D), got shape %r" % (key, shape))
        if shape != tuple(y.shape):
            raise ValueError("my_data['%s'] has shape %r, my_data['y'] %r" % (key, shape, tuple(y.shape)))
        if key == 'weight':
            # (one reduction where the weight lives; NaN fails the first comparison)
            t = getattr(mask, "tensor", mask)
            if torch is not None and torch.is_tensor(t):
                v = t.to(torch.uint8) if t.dtype == torch.bool else t
                ok = bool(((v >= 0) & (v < float("inf"))).all())
            else:
                with np.errstate(invalid="ignore"):
                    a = np.asarray(t)
                    ok = bool(np.all((a >= 0) & (a < np.inf)))
            if not ok:
                raise ValueError("every entry of my_data['weight'] must be finite and >= 0 (0 = not observed): a weight is "
                                 "never clamped")
        if self.Hprime > 16:
            raise _lib.HipError("%s: the %s E-step holds H' <= 16 candidates, got %d"
                                % (type(self).__name__, self._OBS_KIND[key], self.Hprime))

    def _weight_resident(self, weight):
        """``weight`` (NumPy, torch or DeviceArray of any real numeric type) as a float64 device tensor with unit column
        stride, and its leading dimension.  A float64 device tensor of that layout is used in place; anything else is
        converted once."""
        t = getattr(weight, "tensor", weight)
        if not torch.is_tensor(t):
            t = self._f64_dev(np.asarray(t))
        return self._record_rows(t.to(device=self.device, dtype=torch.float64))

    def _record_rows(self, t):
        """An (N, D) observation record on the device with unit column stride (copied if it has another), and its leading
        dimension."""
        D = t.shape[1]
        if t.stride(1) != 1 or t.stride(0) < D:
            t = t.contiguous()
        return t, int(self._row_stride(t, D))

    def _weighted_prepare(self, Y, Wg, ldo, mu=None, x0=False):
        """pm_weighted_prepare_f64: (Xw = omega x, Om = omega, X0 = x or None, sum omega x^2, D_n, 1/2 sum log omega per row), x =
        y - mu where omega != 0 and 0 elsewhere."""
        N, D = Y.shape
        Xw, Om = self._buf("wgt_xw", (N, D)), self._buf("wgt_om", (N, D))
        X0 = self._buf("wgt_x0", (N, D)) if x0 else None
        xn2 = self._buf("wgt_xn2", (N,))
        dn = torch.empty(N, dtype=torch.int32, device=self.device)
        logw = torch.empty(N, dtype=torch.float64, device=self.device)
        mu_d = self._mu_dev(mu)
        self._call("weighted_prepare", "pm_weighted_prepare_f64", _ptr(Y), max(int(Y.stride(0)), D), _ptr(Wg), ldo, _ptr(mu_d),
                   N, D, _ptr(Xw), D, _ptr(Om), D, _ptr(X0), D, _ptr(xn2), _ptr(dn), _ptr(logw), self._stream())
        return Xw, Om, X0, xn2, dn, logw * 0.5

    def _mask_resident(self, mask):
        """``mask`` (NumPy, torch or DeviceArray; bool, uint8 or numeric, non-zero = observed) as a uint8 device tensor with
        unit column stride, and its leading dimension.  A uint8 / bool device tensor of that layout is used in place."""
        t = getattr(mask, "tensor", mask)
        if not torch.is_tensor(t):
            t = torch.from_numpy(np.ascontiguousarray(np.asarray(t) != 0).view(np.uint8))
        t = t.to(self.device)
        if t.dtype == torch.bool:
            t = t.view(torch.uint8)
        elif t.dtype != torch.uint8:
            t = (t != 0).view(torch.uint8)
        return self._record_rows(t)

    def _masked_prepare(self, Y, M, ldm, mu=None):
        """pm_masked_prepare_f64: (X0 = m ? y - mu : 0, Mf = m ? 1 : 0, |X0|^2 per row, D_n per row)."""
        N, D = Y.shape
        X0, Mf = self._buf("mask_x0", (N, D)), self._buf("mask_mf", (N, D))
        xn2 = self._buf("mask_xn2", (N,))
        dn = torch.empty(N, dtype=torch.int32, device=self.device)
        mu_d = self._mu_dev(mu)
        self._call("masked_prepare", "pm_masked_prepare_f64", _ptr(Y), max(int(Y.stride(0)), D), _ptr(M), ldm, _ptr(mu_d), N, D,
                   _ptr(X0), D, _ptr(Mf), D, _ptr(xn2), _ptr(dn), self._stream())
        return X0, Mf, xn2, dn

    def _masked_dense(self, X0, Mf, Wt):
        """The terms that are dense over H, as two products of the one-kernel GEMM: b = X0 . W and diag G_n = Mf . (W o W)."""
        N, H = X0.shape[0], self.H
        b = self._gemm_nt(X0, Wt, self._buf("mask_b", (N, H)), "masked_gemm")
        g = self._gemm_nt(Mf, (Wt * Wt).contiguous(), self._buf("mask_g", (N, H)), "masked_gemm")
        return b, g

    def _obs_prepare(self, Y, obs, mu=None, x0=False):
        """The record of ``obs`` on the device and the prepare kernel of its kind: ``(R, ldr, Xa, Xb, X0, xn2, dn, logw)`` -- the
        record and its leading dimension; the two operands of ``_masked_dense`` (mask: x and m, weight: omega x and omega);
        x itself (weight: only with ``x0``); |x|^2 (omega-weighted) and D_n per row; weight: 1/2 sum log omega per row, else
        None."""
        if obs[0] == 'weight':
            R, ldr = self._weight_resident(obs[1])
            return (R, ldr) + self._weighted_prepare(Y, R, ldr, mu, x0)
        R, ldr = self._mask_resident(obs[1])
        X0, Mf, xn2, dn = self._masked_prepare(Y, R, ldr, mu)
        return R, ldr, X0, Mf, X0, xn2, dn, None

    def _log_likelihood_masked(self, model_params, my_data, per_datapoint, exact):
        """``log_likelihood`` with ``my_data['mask']``: log sum_{s in K_n} p(s, y_obs,n), the per-row constant c0 + D_n c1; with
        ``my_data['weight']`` the constant is c0 + D_n c1 + 1/2 sum_{weight > 0} log weight."""
        y, obs = my_data['y'], self._observation(my_data)
        self._masked_admit(y, obs[1], exact, key=obs[0])
        N = int(y.shape[0])
        if N == 0:
            return np.empty(0) if per_datapoint else self._sum_over_ranks(0.0)
        with self._evaluation():
            out = self._obs_estep(dict(model_params), y, obs)
            dn, c0, c1 = out["dn"], out["c0"], out["c1"]
            logw = out["logw"].cpu().numpy() if out.get("logw") is not None else None      # (weights: 1/2 sum log omega)
            rows, total = self._rows_lse(out["logpj"], 1.0, per_datapoint)
            if per_datapoint:
                rows = rows.cpu().numpy() + (c0 + dn.cpu().numpy().astype(np.float64) * c1)
                return rows if logw is None else rows + logw
            # (the rows' sum in pm_rows_lse_f64's fixed order; sum_n D_n exactly, in integers)
            local = float(total.cpu()[0]) + N * c0 + int(dn.sum(dtype=torch.int64)) * c1
            if logw is not None:
                local += float(np.sum(logw))
        return self._sum_over_ranks(local)

    # ---- the enumeration entries --------------------------------------------------------------
    def _exact_upload(self, arrays):
        """The arrays of the ``_loglik_exact`` hook (or of ``_exact_linear``) as float64 device tensors, None kept."""
        return {k: (torch.from_numpy(np.array(v, dtype=np.float64, order="C")).to(self.device) if v is not None else None)
                for k, v in arrays.items()}

    def _exact_entry(self, model_params, what):
        """The ``_loglik_exact`` hook as a call: ``(kind, arrays, entry)``.  ``entry(call, Yp, ld, n, *out)`` runs
        ``call(name, Yp, ld, <parameters>, n, D, H, *out, stream)`` with the entry name and the parameter arguments of the
        hook's kind for ``what`` -- 'loglik' (pm_loglik_exact_*), 'recon' (pm_recon_exact_*), 'encode' (E[s]: the linear
        kind's reconstruction entry, pm_encode_exact_mca_f64) or 'infer' (pm_infer_exact_*: the arguments of 'recon')."""
        kind, arrays, sc = self._loglik_exact(model_params)
        dev = self._exact_upload(arrays)
        p, dbl, ll = (lambda k: _ptr(dev.get(k))), ctypes.c_double, what == "loglik"
        name = "pm_encode_exact_mca_f64" if (what == "encode" and kind == "mca") else \
            "pm_%s_exact_%s_f64" % ({"loglik": "loglik", "infer": "infer"}.get(what, "recon"), kind)

        if kind == "lin":
            args = [p("mu"), p("P"), p("G"), p("logp"), p("values"), int(arrays["values"].shape[0])] \
                + ([dbl(sc["cst"]), dbl(sc["qcoef"])] if ll else [])
        elif kind == "mca":
            args = [p("Wrho"), dbl(sc["inv_rho"]), int(sc["signed"]), dbl(sc["lp1"]), dbl(sc["lp0"]), dbl(sc["inv_s2"])]
        else:
            args = [p("P")] + ([p("wdiag"), p("Lw")] if ll else []) + [p("M"), p("Psi"), p("mu"), p("logp")]
        if ll and kind != "lin":
            args.append(dbl(sc["cst"]))

        def entry(call, Yp, ld, n, *out, dev=dev):         # (``dev`` keeps the uploads behind ``args`` alive)
            call(name, Yp, ld, *args, n, self.D, self.H, *out, self._stream())
        return kind, arrays, entry

    def _exact_limits(self, entry, ldo):
        """The limits first, before the data reaches the device or anything is launched: with no rows the entry checks its
        arguments (PM_ERANGE past a limit -> HipError) and returns.  Not a launch: it does not go through the timer."""
        probe = torch.empty(1, dtype=torch.float64, device=self.device)
        entry(lambda name, *a: _lib.call(name, *a, det=self.deterministic), None, self.D, 0, None, ldo, _ptr(probe))

    def _exact_rows(self, label, entry, y, out):
        """The reconstruction or encode ``entry`` over the resident rows of ``y`` into ``out`` (N, ldo), which it returns."""
        Y = self._resident(y)["Y"]
        N, D = Y.shape
        lib = _lib.load(self.deterministic)
        work = torch.empty(max(int(lib.pm_recon_exact_work_len(N, self.H, D)), 1), dtype=torch.float64, device=self.device)
        entry(lambda name, *a: self._call(label, name, *a), _ptr(Y), max(int(Y.stride(0)), D), N, _ptr(out), out.shape[1],
              _ptr(work))
        return out

    def _log_likelihood_exact(self, model_params, my_data, per_datapoint):
        with self._evaluation(rows_gemm=False):
            Y = self._resident(my_data['y'])["Y"]
            N, D = Y.shape[0], self.D
            _, _, entry = self._exact_entry(dict(model_params), "loglik")
            lib = _lib.load(self.deterministic)
            work = torch.empty(max(int(lib.pm_loglik_exact_work_len(N, self.H)), 1), dtype=torch.float64, device=self.device)
            total = torch.empty(1, dtype=torch.float64, device=self.device)
            rows = torch.empty(N, dtype=torch.float64, device=self.device) if per_datapoint else None
            entry(lambda name, *a: self._call("loglik_exact", name, *a), _ptr(Y) if N else None,
                  max(int(Y.stride(0)), D) if N else D, N, _ptr(rows), _ptr(work), _ptr(total))
            if per_datapoint:
                return rows.cpu().numpy()
            local = float(total.cpu()[0])
        return self._sum_over_ranks(local)

    def _reconstruct_exact(self, model_params, y, N):
        """The (N, D) device tensor of ``reconstruct(exact=True)``, from the ``_loglik_exact`` hook's ``(kind,
        arrays, scalars)``: 'lin' -- E[s] by pm_recon_exact_lin_f64, then mu + E[s] W^T through ``_recon_product``; 'gsc' --
        E[s o z] by pm_recon_exact_gsc_f64 and the same product with W; 'mca' -- Yhat itself by pm_recon_exact_mca_f64."""
        D, H = self.D, self.H
        kind, arrays, entry = self._exact_entry(model_params, "recon")
        mu = self._nonzero_mu(arrays.get("mu")) if kind == "lin" else None
        Kp = D if kind == "mca" else (H + (1 if mu is not None else 0) + 7) // 8 * 8
        self._exact_limits(entry, Kp)
        if kind == "mca":
            return self._exact_rows("recon_exact", entry, y, torch.empty((N, D), dtype=torch.float64, device=self.device))
        es = torch.zeros((N, Kp), dtype=torch.float64, device=self.device)
        if mu is not None:
            es[:, H] = 1.0
        return self._recon_product(self._exact_rows("recon_exact", entry, y, es), model_params['W'], mu)
