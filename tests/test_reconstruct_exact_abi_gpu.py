"""pm_recon_exact_* (include/prosper_hip.h) through the C ABI itself: padded leading dimensions on both sides, a
base pointer of Y that is 8 bytes off the 16-byte grid, E[s] / E[s o z] / Yhat against NumPy sums over every state to the
project's 1e-11 (relative to the row's largest entry), more rows than one row block of the entries' walk, and a padded
output buffer whose columns past the row width and rows past N stay untouched."""
import ctypes
import itertools

import numpy as np
import pytest

import recon_reference as R
from test_reconstruct_gpu import _problem

pytestmark = pytest.mark.gpu

RTOL = 1e-11
SENTINEL = -12345.678


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _up(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


def _padded_y(Y, ldy, dev):
    """Y in a buffer with row stride ldy whose first row starts 8 bytes past a 16-byte boundary."""
    import torch
    N, D = Y.shape
    buf = torch.full((N * ldy + 3,), float("nan"), dtype=torch.float64, device=dev)
    off = 1 if buf.data_ptr() % 16 == 0 else 2
    view = buf[off:off + N * ldy].view(N, ldy)
    view[:, :D] = torch.from_numpy(Y).to(dev)
    assert view.data_ptr() % 16 == 8
    return buf, view


def _run(dev, m, p, Y, width, ldy, ldo, extra_rows, det=False):
    """The model's hook arrays through the entry of its kind; returns the whole padded output (N + extra_rows, ldo)."""
    import torch
    from prosper_amd import _lib
    lib = _lib.load(det)
    N, D = Y.shape
    H = m.H
    kind, arrays, sc = m._loglik_exact({k: np.array(v, copy=True) for k, v in p.items()})
    d = {k: _up(v, dev) for k, v in arrays.items() if v is not None}
    keep, Yd = _padded_y(Y, ldy, dev)
    out = torch.full((N + extra_rows, ldo), SENTINEL, dtype=torch.float64, device=dev)
    wl = int(lib.pm_recon_exact_work_len(N, H, D))
    assert wl >= 1
    work = torch.empty(wl, dtype=torch.float64, device=dev)
    dbl = ctypes.c_double
    if kind == "lin":
        mu = _ptr(d["mu"]) if "mu" in d else None
        rc = lib.pm_recon_exact_lin_f64(_ptr(Yd), ldy, mu, _ptr(d["P"]), _ptr(d["G"]), _ptr(d["logp"]), _ptr(d["values"]),
                                        int(arrays["values"].shape[0]), N, D, H, _ptr(out), ldo, _ptr(work), None)
    elif kind == "mca":
        rc = lib.pm_recon_exact_mca_f64(_ptr(Yd), ldy, _ptr(d["Wrho"]), dbl(sc["inv_rho"]), int(sc["signed"]), dbl(sc["lp1"]),
                                        dbl(sc["lp0"]), dbl(sc["inv_s2"]), N, D, H, _ptr(out), ldo, _ptr(work), None)
    else:
        rc = lib.pm_recon_exact_gsc_f64(_ptr(Yd), ldy, _ptr(d["P"]), _ptr(d["M"]), _ptr(d["Psi"]), _ptr(d["mu"]),
                                        _ptr(d["logp"]), N, D, H, _ptr(out), ldo, _ptr(work), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check(tag, full, want, N, width):
    got = full[:N, :width]
    scale = np.abs(want).max(axis=1)
    err = float((np.abs(got - want).max(axis=1) / np.where(scale > 0, scale, 1.0)).max())
    print("recon exact ABI %-30s error relative to the row's largest entry %.3e (bound %.1e)" % (tag, err, RTOL))
    assert err <= RTOL, (tag, err)
    assert np.all(full[:N, width:] == SENTINEL), "columns past the row width were written"
    assert np.all(full[N:] == SENTINEL), "rows past N were written"


def _lin_marginals(Y, W, sigma, values, logp, mu=None):
    """E[s] (N, H) by enumeration: the posterior of enum_linear, times the states."""
    H = W.shape[1]
    values = np.asarray(values, dtype=np.float64)
    idx = np.array(list(itertools.product(range(len(values)), repeat=H)))
    S = values[idx]
    with np.errstate(invalid="ignore"):
        lp = np.asarray(logp, dtype=np.float64)[idx].sum(axis=1)
    keep = np.isfinite(lp)
    S, lp = S[keep], lp[keep]
    means = S @ W.T + (0.0 if mu is None else np.asarray(mu)[None, :])
    r2 = ((Y[:, None, :] - means[None, :, :]) ** 2).sum(-1)
    return R.softmax_rows(lp[None, :] - 0.5 * r2 / sigma ** 2) @ S


def _gsc_marginals(p, Y):
    """E[s o z] (N, H) by enumeration with dense NumPy algebra per support (the terms of recon_reference.gsc_state_terms)."""
    W, mu, Psi = p["W"], np.asarray(p["mu"], dtype=np.float64), p["psi_sq"]
    D, H = W.shape
    pi = np.broadcast_to(np.asarray(p["pi"], dtype=np.float64), (H,))
    Sig = R._gsc_sigma(p, D)
    logps, kaps = [], []
    for s in itertools.product([0, 1], repeat=H):
        a = np.nonzero(s)[0]
        lp = np.log(pi[a]).sum() + np.log(1 - np.delete(pi, a)).sum()
        Wa, Pa = W[:, a], Psi[np.ix_(a, a)]
        C = Sig + Wa @ Pa @ Wa.T
        r = Y - (Wa @ mu[a])[None, :]
        Cr = np.linalg.solve(C, r.T)
        logps.append(lp - 0.5 * np.linalg.slogdet(C)[1] - 0.5 * (r * Cr.T).sum(axis=1))
        k = np.zeros((len(Y), H))
        k[:, a] = mu[a][None, :] + (Pa @ Wa.T @ Cr).T
        kaps.append(k)
    q = R.softmax_rows(np.stack(logps, axis=1))
    return sum(q[:, i:i + 1] * kaps[i] for i in range(len(kaps)))


@pytest.mark.parametrize("name,H,N", [("bsc", 6, 300), ("bsc_mu", 11, 70), ("tsc", 7, 40), ("dsc4", 6, 40)])
def test_linear_marginals(dev, name, H, N):
    D = 12
    m, p, Y, _, _ = _problem(name, np.random.RandomState(60 + H), D, H, N, 3, 2)
    if name == "tsc":
        values, lp = [-1., 0., 1.], np.log([p["pi"] / 2, 1 - p["pi"], p["pi"] / 2])
    elif name == "dsc4":
        values, lp = m.states, np.log(p["pi"])
    else:
        values, lp = [0., 1.], np.log([1 - p["pi"], p["pi"]])
    want = _lin_marginals(Y, p["W"], p["sigma"], values, lp, mu=p.get("mu"))
    full = _run(dev, m, p, Y, H, D + 5, H + 3, 4)
    _check("%s H=%d N=%d" % (name, H, N), full, want, N, H)
    again = _run(dev, m, p, Y, H, D + 1, H, 0, det=True)          # other strides, the other library: the same bits
    assert np.array_equal(again.view(np.uint64), np.ascontiguousarray(full[:N, :H]).view(np.uint64))


@pytest.mark.parametrize("kind,H,N", [("gsc_scalar", 5, 300), ("gsc_full", 7, 70)])
def test_gsc_marginals(dev, kind, H, N):
    D = 10
    m, p, Y, _, _ = _problem(kind, np.random.RandomState(70 + H), D, H, N, 3, 2)
    full = _run(dev, m, p, Y, H, D + 3, H + 2, 3)
    _check("%s H=%d N=%d" % (kind, H, N), full, _gsc_marginals(p, Y), N, H)
    again = _run(dev, m, p, Y, H, D, H, 0, det=True)
    assert np.array_equal(again.view(np.uint64), np.ascontiguousarray(full[:N, :H]).view(np.uint64))


@pytest.mark.parametrize("name,D,H,N", [("mca", 12, 6, 70), ("mmca", 70, 7, 20)])
def test_mca_rows(dev, name, D, H, N):
    m, p, Y, _, enum = _problem(name, np.random.RandomState(80 + H), D, H, N, 3, 2)
    full = _run(dev, m, p, Y, D, D + 7, D + 2, 5)
    _check("%s D=%d H=%d N=%d" % (name, D, H, N), full, enum(Y), N, D)
    again = _run(dev, m, p, Y, D, D + 1, D, 0, det=True)
    assert np.array_equal(again.view(np.uint64), np.ascontiguousarray(full[:N, :D]).view(np.uint64))
