"""k-means++ seeding (D^2 sampling; Arthur & Vassilvitskii 2007) of the mixture models on the device.

``kmeanspp`` draws H rows of the data, each with probability proportional to its squared distance to the nearest row drawn
so far: H dependent passes over the resident shard (pm_seed_update_f64) and a weighted draw per pass (pm_seed_pick_f64), every
sum in the pinned order include/prosper_hip.h documents, so that tests/seeding_reference.py reproduces indices and bits.  There
is no CPU fallback.
"""
import ctypes

import numpy as np

from . import parallel
from .. import _lib

try:
    import torch
except Exception:  # pragma: no cover
    torch = None


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def check_uniforms(uniforms, H):
    """``uniforms`` as a host (H,) float64 array: another shape, a value outside [0, 1) or a NaN raises ``ValueError``."""
    u = getattr(uniforms, "tensor", uniforms)
    if torch is not None and torch.is_tensor(u):
        u = u.detach().cpu().numpy()
    u = np.asarray(u, dtype=np.float64)
    if u.shape != (H,):
        raise ValueError("kmeanspp: uniforms must have shape (%d,), got %r" % (H, u.shape))
    if not ((u >= 0.0) & (u < 1.0)).all():          # (a NaN fails both compares)
        raise ValueError("kmeanspp: uniforms must lie in [0, 1)")
    return u


def _resident(Y, device):
    """The shard as a float64 device tensor with unit column stride and an even row stride of its own or a copy: a float64
    device tensor with unit column stride is used in place, anything else is converted once."""
    y = getattr(Y, "tensor", Y)
    if torch.is_tensor(y):
        if y.dim() != 2:
            raise ValueError("kmeanspp: Y must be (my_N, D), got %r" % (tuple(y.shape),))
        if y.is_cuda and y.dtype == torch.float64 and (y.shape[0] <= 1 or y.stride(0) >= y.shape[1]) \
                and (y.shape[1] == 1 or y.stride(1) == 1):
            return y
        return y.to(device=device, dtype=torch.float64).contiguous()
    y = np.asarray(y)
    if y.ndim != 2:
        raise ValueError("kmeanspp: Y must be (my_N, D), got %r" % (y.shape,))
    return torch.from_numpy(np.ascontiguousarray(y, dtype=np.float64)).to(device)


def kmeanspp(Y, H, seed=None, uniforms=None, comm=parallel.COMM_WORLD, device=False, deterministic=False):
    """H rows of the data by D^2 sampling.  ``Y``: this rank's shard (my_N, D) -- NumPy, a torch tensor or a ``DeviceArray``,
    float32 or float64.  Returns ``(centres (H, D) float64, indices (H,) int64, potential (H,) float64)``: the chosen rows,
    their global row numbers (the ranks' shards in rank order) and, per round, the sum over all datapoints of the squared
    distance to the nearest centre chosen so far (non-increasing).  ``device=True`` leaves ``centres`` on the device (a
    ``DeviceArray``).  ``deterministic``: run libprosper_hip_det.so; the kernels hold no atomics, so the bits are the same.

    Randomness: ``uniforms`` (H,) in [0, 1), or ``torch.rand(H)`` (float64) from a device generator seeded with ``seed``
    (``None``: fresh entropy), drawn on rank 0 and broadcast.  Round 0 takes row min(floor(u_0 N), N - 1) of the global N;
    round h >= 1 the first row whose running sum of distances exceeds t = u_h S (include/prosper_hip.h: the block rule
    depends on my_N, so another sharding of the same data may draw another row where t falls within rounding of a boundary).
    With ``uniforms`` the result is a pure function of the inputs.

    One rank: the H rounds are enqueued without a host synchronisation -- the pick kernel leaves the index in device memory
    and the next update reads the centre row through it -- and the results are checked once, after the download.  Several
    ranks (or PM_FORCE_COLLECTIVES=1): per round one all-gather of the ranks' potentials S_r; the total is ((S_0 + S_1) + ...)
    in rank order; the owner is the first rank whose running total exceeds t (if rounding leaves none, the last rank with S_r >
    0), draws with t minus the running total before it and broadcasts the row.

    ``ValueError`` before any launch: H < 1 or H > N, ``uniforms`` of another shape or outside [0, 1), both ``seed`` and
    ``uniforms``.  After the rounds: fewer than H distinct rows (the potential reaches 0 first; the message names the round)
    and a non-finite potential (NaN or inf in the data)."""
    if seed is not None and uniforms is not None:
        raise ValueError("kmeanspp: give seed or uniforms, not both")
    H = int(H)
    shape = tuple(getattr(Y, "tensor", Y).shape)
    if len(shape) != 2 or shape[1] < 1:
        raise ValueError("kmeanspp: Y must be (my_N, D) with D >= 1, got %r" % (shape,))
    my_N, D = int(shape[0]), int(shape[1])
    counts = [int(c) for c in comm.allgather(my_N)]
    N = sum(counts)
    if H < 1 or H > N:
        raise ValueError("kmeanspp: H = %d outside 1 .. N = %d" % (H, N))
    if uniforms is not None:
        u = check_uniforms(uniforms, H)
    if torch is None or not torch.cuda.is_available():
        raise _lib.HipError("kmeanspp needs a HIP device: there is no CPU fallback")
    dev = torch.device("cuda", torch.cuda.current_device())
    if uniforms is None:
        u = None
        if comm.rank == 0:
            g = torch.Generator(device=dev)
            g.manual_seed(int(seed)) if seed is not None else g.seed()
            u = torch.rand(H, generator=g, device=dev, dtype=torch.float64).cpu().numpy()
        u = comm.bcast(u)
    Yd = _resident(Y, dev)
    ldy = int(Yd.stride(0)) if my_N > 1 else max(D, int(Yd.stride(0)))
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    lib = _lib.load(deterministic)

    def call(name, *a):
        _lib.call(name, *a, det=deterministic)

    dist = torch.empty(max(my_N, 1), dtype=torch.float64, device=dev)
    work = torch.empty(int(lib.pm_seed_work_len(my_N)), dtype=torch.float64, device=dev)
    i0 = min(int(np.floor(u[0] * N)), N - 1)
    if comm._solo():
        host_idx = np.full(H, -1, dtype=np.int64)
        host_idx[0] = i0
        idx = torch.from_numpy(host_idx).to(dev)
        pot = torch.empty(H, dtype=torch.float64, device=dev)
        for h in range(H):
            if h:
                call("pm_seed_pick_f64", _ptr(dist), my_N, _ptr(work), None, 0.0, float(u[h]),
                     ctypes.c_void_p(idx.data_ptr() + 8 * h), st)
            call("pm_seed_update_f64", _ptr(Yd), ldy, my_N, D, _ptr(Yd), ldy, my_N, ctypes.c_void_p(idx.data_ptr() + 8 * h),
                 int(h == 0), _ptr(dist), _ptr(work), ctypes.c_void_p(pot.data_ptr() + 8 * h), st)
        centres = torch.empty((H, D), dtype=torch.float64, device=dev)
        call("pm_seed_gather_f64", _ptr(Yd), ldy, my_N, D, _ptr(idx), H, _ptr(centres), D, st)
        indices, potential = idx.cpu().numpy(), pot.cpu().numpy()        # (the one synchronisation)
        _check(indices, potential)
        if device:
            from ..em.camodels._device import DeviceArray
            return DeviceArray(centres), indices, potential
        return centres.cpu().numpy(), indices, potential

    # ---- several ranks: two small collectives per round --------------------------------------------------------------
    rank = comm.rank
    first_row = int(np.sum(counts[:rank]))
    indices = np.full(H, -1, dtype=np.int64)
    potential = np.zeros(H)
    centres = np.zeros((H, D))
    row_d = torch.empty((1, D), dtype=torch.float64, device=dev)
    dead_d = torch.full((1,), -1, dtype=torch.int64, device=dev)
    pick_d = torch.empty(1, dtype=torch.int64, device=dev)
    S_d = torch.empty(1, dtype=torch.float64, device=dev)
    total_d = torch.empty(1, dtype=torch.float64, device=dev)
    sums = [0.0] * comm.size
    for h in range(H):
        owner, local = -1, -1
        if h == 0:
            owner = int(np.searchsorted(np.cumsum(counts), i0, side="right"))
            local = i0 - int(np.sum(counts[:owner]))
        else:
            total = 0.0
            for s in sums:
                total = total + s
            if total != 0.0:
                t = float(u[h]) * total
                run = 0.0
                for r, s in enumerate(sums):
                    before = run
                    run = run + s
                    if run > t:
                        owner, before_owner = r, before
                        break
                if owner < 0:
                    positive = [r for r, s in enumerate(sums) if s > 0.0]
                    if positive:
                        owner = positive[-1]
                        before_owner = 0.0
                        for s in sums[:owner]:
                            before_owner = before_owner + s
                if owner == rank:
                    total_d.copy_(torch.tensor([total], dtype=torch.float64))
                    call("pm_seed_pick_f64", _ptr(dist), my_N, _ptr(work), _ptr(total_d), -before_owner, float(u[h]),
                         _ptr(pick_d), st)
                    local = int(pick_d.cpu()[0])
        msg = None
        if owner == rank:
            msg = (first_row + local, Yd[local].cpu().numpy()) if local >= 0 else (-1, None)
        gidx, row = comm.bcast(msg, root=owner) if owner >= 0 else (-1, None)
        indices[h] = gidx
        if gidx >= 0:
            centres[h] = row
            row_d.copy_(torch.from_numpy(np.ascontiguousarray(row, dtype=np.float64)[None, :]))
        if my_N:
            call("pm_seed_update_f64", _ptr(Yd), ldy, my_N, D, _ptr(row_d), D, 1, None if gidx >= 0 else _ptr(dead_d),
                 int(h == 0), _ptr(dist), _ptr(work), _ptr(S_d), st)
            mine = float(S_d.cpu()[0])
        else:
            mine = 0.0
        sums = [float(s) for s in comm.allgather(mine)]
        total = 0.0
        for s in sums:
            total = total + s
        potential[h] = total
    _check(indices, potential)
    if device:
        from ..em.camodels._device import DeviceArray
        return DeviceArray(torch.from_numpy(centres).to(dev)), indices, potential
    return centres, indices, potential


def _check(indices, potential):
    """The one look at the downloaded results."""
    if not np.isfinite(potential).all():
        raise ValueError("kmeanspp: the potential is not finite from round %d on (NaN or inf in the data)"
                         % int(np.nonzero(~np.isfinite(potential))[0][0]))
    if (indices < 0).any():
        h = int(np.nonzero(indices < 0)[0][0])
        raise ValueError("kmeanspp: the data has only %d distinct rows: the potential reached 0 before round %d, no centre "
                         "left to draw" % (h, h))
