"""``BSC_ET.exact_step`` and ``model.exact = True`` on the device: against the project's own truncated step at
H' = gamma = H, against the NumPy enumeration of tests/exact_em_reference.py, against ``log_likelihood(exact=True)``, the
monotone free energy, the dispatch through ``step`` / ``EM.run``, what an exact step leaves untouched, reproducibility,
partial data and two ranks.  Tolerances: RTOL_STEP for the parameters (W relative to its largest entry), 1e-11 for L."""
import numpy as np
import pytest

import exact_em_reference as X

pytestmark = pytest.mark.gpu

RTOL_STEP = 1e-8
RTOL_L = 1e-11


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def _bsc(D, H, Hp=None, g=None, to_learn=("W", "pi", "sigma"), det=False):
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    m = BSC_ET(D, H, Hp or min(H, 3), g or min(H, 2), to_learn=list(to_learn))
    m.deterministic = det
    return m


def _logged(fn, keys=("L", "N", "N_use")):
    from prosper_amd.utils.datalog import dlog, StoreInMemory
    h = dlog.set_handler(keys, StoreInMemory)
    try:
        out = fn()
    finally:
        dlog.remove_handler(h)
    return out, {k: [float(np.asarray(x)) for x in v] for k, v in h.tables.items() if k in keys}


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max())


def _compare(tag, new, log, ref, rL, rN, learn_mu):
    errs = {"W": _rel(new["W"], ref["W"]), "pi": abs(new["pi"] / ref["pi"] - 1), "sigma": abs(new["sigma"] / ref["sigma"] - 1),
            "mu": _rel(new["mu"], ref["mu"]) if learn_mu else float(np.abs(np.asarray(new["mu"]) - ref["mu"]).max()),
            "L": abs(log["L"][-1] / rL - 1)}
    print("exact EM %-40s " % tag + "  ".join("%s %.2e" % kv for kv in errs.items()))
    assert max(errs["W"], errs["pi"], errs["sigma"], errs["mu"]) <= RTOL_STEP, (tag, errs)
    assert errs["L"] <= RTOL_L, (tag, errs)
    assert log["N_use"][-1] == rN and log["N"][-1] == rN


def _same(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in ("W", "pi", "sigma", "mu"))


_PROBLEMS = {}


def _problem(D, H, N, mu=False):
    """One problem (and its NumPy steps) per shape for the whole module; start pi = 0.25, where the truncated M-step's
    A_pi_gamma at gamma = H is 1.0 to the bit and ``Ncut_factor = 1`` keeps all N datapoints there too."""
    key = (D, H, N, mu)
    if key not in _PROBLEMS:
        params, Y = X.problem(np.random.RandomState(100 * H + N), D, H, N, pi=0.25, mu=mu)
        params["pi"] = 0.25
        _PROBLEMS[key] = (params, Y, {})
    return _PROBLEMS[key]


def _reference(D, H, N, mu, an, to_learn):
    params, Y, cache = _problem(D, H, N, mu)
    key = (an["T"], bool(an["anneal_prior"]), tuple(to_learn))
    if key not in cache:
        cache[key] = X.step(X.Anneal(T=an["T"], anneal_prior=an["anneal_prior"]), params, Y, to_learn)
        assert cache[key][1]["cond"] < 1e6
    return cache[key]


ANNEALS = [dict(T=1.0), dict(T=1.7, anneal_prior=False), dict(T=1.7, anneal_prior=True), dict(T=1.0, Ncut_factor=1.0)]


@pytest.mark.parametrize("an", ANNEALS, ids=["T1", "T1.7", "T1.7-prior", "T1-Ncut1"])
@pytest.mark.parametrize("learn_mu", [False, True], ids=["", "mu"])
@pytest.mark.parametrize("H", [6, 10])
def test_against_truncated_step_at_full_width(dev, H, learn_mu, an):
    """The truncated step at H' = gamma = H scores every state: same start, same data, W, pi, sigma, mu, L and N_use.  H = 10
    is the largest the truncated step takes at full width: at H = 11 the pair lists of its 2036 multi-cause states need 205 KB
    of LDS in pm_bsc_mstep_rows_f64 (160 KB; PM_ERANGE), and the 16-lane kernels stop at H = 8."""
    D, N = 16, 200
    to_learn = ("W", "pi", "sigma") + (("mu",) if learn_mu else ())
    params, Y, _ = _problem(D, H, N, learn_mu)
    _, rlog = _reference(D, H, N, learn_mu, X.Anneal(**an), to_learn)       # (the condition number, on the reference)
    anneal = X.Anneal(**an)
    cp = lambda: {k: np.array(v, copy=True) if np.ndim(v) else v for k, v in params.items()}
    ref, tl = _logged(lambda: _bsc(D, H, H, H, to_learn).step(anneal, cp(), {"y": Y}))
    assert tl["N_use"][-1] == N
    new, log = _logged(lambda: _bsc(D, H, to_learn=to_learn).exact_step(anneal, cp(), {"y": Y}))
    _compare("H=%d %s vs truncated" % (H, an), new, log, ref, tl["L"][-1], N, learn_mu)


@pytest.mark.parametrize("learn_mu", [False, True], ids=["", "mu"])
def test_against_enumeration_H13(dev, learn_mu):
    """H = 13: 8 chunks, R = 4, three pinned sweeps -- past what the truncated step reaches."""
    D, H, N = 16, 13, 120
    to_learn = ("W", "pi", "sigma") + (("mu",) if learn_mu else ())
    params, Y, _ = _problem(D, H, N, learn_mu)
    an = X.Anneal(T=1.3, anneal_prior=True)
    ref, rlog = _reference(D, H, N, learn_mu, an, to_learn)
    new, log = _logged(lambda: _bsc(D, H, to_learn=to_learn).exact_step(an, dict(params), {"y": Y}))
    _compare("H=13 vs NumPy", new, log, ref, rlog["L"], N, learn_mu)


def test_L_is_the_exact_log_likelihood(dev):
    D, H, N = 16, 10, 200
    params, Y, _ = _problem(D, H, N)
    m = _bsc(D, H)
    _, log = _logged(lambda: m.exact_step(X.Anneal(T=1.0), dict(params), {"y": Y}))
    ll = m.log_likelihood(dict(params), {"y": Y}, exact=True) / N
    print("exact EM L %.15g  log_likelihood(exact=True)/N %.15g  rel %.2e" % (log["L"][-1], ll, abs(log["L"][-1] / ll - 1)))
    assert abs(log["L"][-1] / ll - 1) <= RTOL_L


def test_free_energy_never_falls(dev):
    """25 exact steps at T = 1: EM's guarantee, with nothing truncated; rounding alone is ~1e-15 |L|."""
    D, H, N = 16, 8, 300
    params, Y = X.problem(np.random.RandomState(8), D, H, N)
    m = _bsc(D, H)
    an = X.Anneal(T=1.0)

    def run():
        p = dict(params)
        for _ in range(25):
            p = m.exact_step(an, p, {"y": Y})
        return p
    _, log = _logged(run)
    L = np.array(log["L"])
    worst = float(((L[1:] - L[:-1]) / np.abs(L[:-1])).min())
    print("exact EM 25 steps: L %.6f -> %.6f, smallest relative change %.2e" % (L[0], L[-1], worst))
    assert len(L) == 25 and worst >= -1e-12 and L[-1] > L[0]


def test_attribute_dispatches_step_and_em_run(dev):
    from prosper_amd.em import EM
    from prosper_amd.em.annealing import LinearAnnealing
    D, H, N = 16, 8, 150
    params, Y = X.problem(np.random.RandomState(9), D, H, N)
    m = _bsc(D, H, det=True)
    m.exact = True
    an = LinearAnnealing(3)
    an['T'] = [(0, 1.5), (1., 1.)]
    an['anneal_prior'] = False
    em = EM(model=m, anneal=an, data={"y": Y}, lparams=dict(params))
    em.run()
    m2 = _bsc(D, H, det=True)
    an2 = LinearAnnealing(3)
    an2['T'] = [(0, 1.5), (1., 1.)]
    an2['anneal_prior'] = False
    p = dict(params)
    while not an2.finished:
        p = m2.exact_step(an2, p, {"y": Y})
        an2.next(0.)
    assert _same(em.lparams, p)
    assert _rel(p["W"], params["W"]) > 1e-6


def test_truncated_steps_untouched(dev):
    """The attribute unset or False changes nothing, and a truncated step after an exact one returns the bits of the truncated
    step alone (deterministic library)."""
    D, H, N = 16, 10, 200
    params, Y = X.problem(np.random.RandomState(11), D, H, N)
    an = X.Anneal(T=1.2)
    data = {"y": Y}

    def trunc(m, steps=3, exact_between=False):
        p = dict(params)
        for i in range(steps):
            p = m.step(an, dict(p), data)
            if exact_between:
                m.exact_step(an, dict(p), data)
                m.exact_step(an, dict(params), {"y": Y[:50].copy()})
        return p
    a = trunc(_bsc(D, H, 5, 3, det=True))
    m = _bsc(D, H, 5, 3, det=True)
    m.exact = False
    assert _same(a, trunc(m))
    assert _same(a, trunc(_bsc(D, H, 5, 3, det=True), exact_between=True))


def test_same_bits_again(dev):
    D, H, N = 16, 13, 120
    params, Y, _ = _problem(D, H, N)
    an = X.Anneal(T=1.3)
    m = _bsc(D, H)
    a = m.exact_step(an, dict(params), {"y": Y})
    assert _same(a, m.exact_step(an, dict(params), {"y": Y}))
    assert _same(a, _bsc(D, H).exact_step(an, dict(params), {"y": Y}))
    assert _same(a, _bsc(D, H, det=True).exact_step(an, dict(params), {"y": Y}))


def test_partial_data(dev):
    """anneal['partial'] = 0.5: the step on the row subset ``select_partial_data`` draws."""
    D, H, N = 16, 8, 150
    params, Y = X.problem(np.random.RandomState(12), D, H, N)
    m = _bsc(D, H)
    np.random.seed(5)
    new, log = _logged(lambda: m.exact_step(X.Anneal(T=1.0, partial=0.5), dict(params), {"y": Y}))
    np.random.seed(5)
    sel = np.sort(np.random.permutation(N)[:75])
    want = _bsc(D, H).exact_step(X.Anneal(T=1.0), dict(params), {"y": Y[sel]})
    assert _same(new, want) and log["N_use"][-1] == 75


def test_two_ranks_over_gloo(dev):
    """tests/exact_em_world2_gpu_worker.py: two processes, a world_size-2 gloo group on the one GPU."""
    import os
    import socket
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    worker = os.path.join(here, "exact_em_world2_gpu_worker.py")
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    procs = []
    for rank in range(2):
        e = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                 RANK=str(rank), WORLD_SIZE="2")
        procs.append(subprocess.Popen([sys.executable, worker], env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                      text=True))
    outs = []
    try:
        for pr in procs:
            outs.append(pr.communicate(timeout=300))
    finally:
        for pr in procs:
            if pr.poll() is None:
                pr.kill()
    for rank, (pr, (out, err)) in enumerate(zip(procs, outs)):
        assert pr.returncode == 0 and ("ok %d" % rank) in out.split("\n"), "rank %d\n%s\n%s" % (rank, out[-2000:], err[-4000:])
