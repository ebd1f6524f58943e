"""Deterministic-reduction mode (`model.deterministic = True`, libprosper_hip_det.so): the reference at a fixed number of ranks
is deterministic, the HIP path sums its M-step statistics with f64 atomics whose order changes from run to run.  In the
deterministic build every addend is rounded to a common quantum first (pm_common.h, PM_Q), so the sums -- and with them every
parameter -- come out bit for bit the same in every run; and because nothing else changes, comparing it with the default build
step by step doubles as a race detector for the atomics (a lost or doubled update is no rounding-level difference)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


class _An(dict):
    crit_params = []

    def __missing__(self, k):
        return 0.0

    def as_dict(self):
        return dict(self)


def _copy(p):
    return {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in p.items()}


def _bsc(shape):
    from oracle import bsc_oracle as O
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    D, H, Hp, g, N = shape
    rng = np.random.RandomState(11)
    W = rng.normal(size=(D, H))
    y = O.generate_bsc_data(W, 2.0 / H, 1.0, N, rng)[0]
    return (lambda: BSC_ET(D, H, Hp, g)), {"W": W + 0.2 * rng.normal(size=(D, H)), "pi": 2.5 / H, "sigma": 1.1}, y, ("W", "pi", "sigma")


def _mca(shape):
    from oracle import mca_oracle as O
    from prosper_amd.em.camodels.mca_et import MCA_ET
    D, H, Hp, g, N = shape
    rng = np.random.RandomState(12)
    W = np.abs(rng.normal(size=(D, H))) * 3 + 0.1
    y = O.generate_mca_data(W, 2.0 / H, 1.0, N, rng)[0]
    return (lambda: MCA_ET(D, H, Hp, g)), {"W": W * rng.uniform(0.9, 1.1, size=W.shape), "pi": 2.5 / H, "sigma": 1.1}, y, ("W", "pi", "sigma")


def _dsc(shape):
    from prosper_amd.em.camodels.dsc_et import DSC_ET
    D, H, Hp, g, N = shape
    rng = np.random.RandomState(13)
    states = np.array([-1.0, 0.0, 1.0, 2.0])
    W = rng.normal(size=(D, H))
    s = states[rng.choice(4, size=(N, H), p=[0.04, 0.88, 0.05, 0.03])]
    y = s @ W.T + rng.normal(size=(N, D))
    return ((lambda: DSC_ET(D, H, Hp, g, states=states.copy())),
            {"W": W + 0.2 * rng.normal(size=(D, H)), "pi": np.array([0.05, 0.85, 0.06, 0.04]), "sigma": 1.1}, y, ("W", "pi", "sigma"))


def _gsc(shape):
    from oracle import gsc_oracle as O
    from prosper_amd.em.camodels.gsc_et import GSC
    D, H, Hp, g, N = shape
    rng = np.random.RandomState(14)
    gt = {"W": rng.normal(size=(D, H)), "pi": np.full(H, 2.0 / H), "mu": np.full(H, 1.5), "psi_sq": np.eye(H), "sigma_sq": 1.0}
    y = O.generate_gsc_data(gt, N, rng)[0]
    p = {"W": gt["W"] + 0.1 * rng.normal(size=(D, H)), "pi": gt["pi"] * 1.1, "mu": gt["mu"] + 0.1 * rng.normal(size=H),
         "psi_sq": np.diag(rng.uniform(0.7, 1.4, size=H)), "sigma_sq": 1.2}
    return (lambda: GSC(D, H, Hp, g, "scalar")), p, y, ("W", "pi", "mu", "psi_sq", "sigma_sq")


def _mmca(shape):
    from oracle import mmca_oracle as O
    from prosper_amd.em.camodels.mmca_et import MMCA_ET
    D, H, Hp, g, N = shape
    rng = np.random.RandomState(16)
    W = rng.normal(size=(D, H)) * 3.0
    y = O.generate_from_hidden(W, rng.random_sample((N, H)) < 2.0 / H) + rng.normal(size=(N, D))
    return (lambda: MMCA_ET(D, H, Hp, g)), {"W": W * rng.uniform(0.9, 1.1, size=W.shape), "pi": 2.4 / H, "sigma": 1.1}, y, ("W", "pi", "sigma")


def _tsc(shape):
    from prosper_amd.em.camodels.tsc_et import TSC_ET
    D, H, Hp, g, N = shape
    rng = np.random.RandomState(17)
    W = rng.normal(size=(D, H)) * 2.0
    s = rng.choice([-1., 0., 1.], size=(N, H), p=[1.0 / H, 1 - 2.0 / H, 1.0 / H])
    y = s @ W.T + rng.normal(size=(N, D))
    return (lambda: TSC_ET(D, H, Hp, g)), {"W": W + 0.2 * rng.normal(size=(D, H)), "pi": 2.4 / H, "sigma": 1.1}, y, ("W", "pi", "sigma")


_CASES = {
    "mmca": (_mmca, (64, 40, 6, 3, 600)), "tsc": (_tsc, (32, 24, 5, 3, 900)),       # the models that inherit the mode
    "bsc_small": (_bsc, (20, 12, 5, 3, 700)), "bsc_fast": (_bsc, (64, 160, 8, 3, 1500)),      # fast: the 16-wavefront kernel's shapes
    "mca": (_mca, (64, 128, 8, 3, 900)), "dsc": (_dsc, (32, 24, 5, 3, 900)), "gsc": (_gsc, (128, 128, 6, 3, 1200)),
    # shapes whose scores GEMM (pm_gemm_nt_f64) would split K in the default build -- a ragged remainder behind whole rounds
    # of the 4-wavefront fused kernel; a shard smaller than one round at a large D (round-5 advisor finding: the slices'
    # atomics were quantised with another kernel family's bounds, or none: the deterministic build does not split there)
    "bsc_splitk": (_bsc, (256, 64, 6, 3, 40000)), "dsc_splitk": (_dsc, (512, 24, 5, 3, 900)),
    # gamma = 5: the quanta's bounds grow with the number of states (the 4-wavefront one-kernel pass; scores GEMM + 16-lane row
    # kernel above H = 256; MCA's 210 states; DSC's 1008 with four values; GSC's G = 6 systems)
    "bsc_g5": (_bsc, (40, 30, 8, 5, 900)), "bsc_g5_two_kernel": (_bsc, (64, 300, 8, 5, 3000)),
    "mca_g5": (_mca, (64, 40, 8, 5, 600)), "dsc_g5": (_dsc, (32, 24, 5, 5, 600)), "gsc_g5": (_gsc, (48, 40, 7, 5, 600)),
}


def _loop(make, p0, y, keys, steps, det, schedule):
    m = make()
    m.deterministic = det
    p, traj = _copy(p0), []
    for it in range(steps):
        p = m.step(_An(schedule(it)), p, {"y": y})
        traj.append({k: np.array(p[k], copy=True) for k in keys})
    return traj


@pytest.mark.parametrize("case", sorted(_CASES))
def test_deterministic_mode_repeats_bit_for_bit(case):
    """The same 50-step EM loop twice (annealing, and for the models that have it a data-truncation phase): every parameter of
    every step identical to the last bit; and the loop stays within rounding of the default build's."""
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU box (MI355X)")
    fn, shape = _CASES[case]
    make, p0, y, keys = fn(shape)
    cut = case.startswith(("bsc", "mca", "dsc"))
    schedule = lambda it: {"T": 1.5 if it < 10 else 1.0, "Ncut_factor": 0.6 if (cut and it >= 30) else 0.0}
    a = _loop(make, p0, y, keys, 50, True, schedule)
    b = _loop(make, p0, y, keys, 50, True, schedule)
    for it, (pa, pb) in enumerate(zip(a, b)):
        for k in keys:
            assert np.array_equal(pa[k], pb[k]), "%s: step %d, %s differs between two deterministic runs" % (case, it, k)
    assert all(np.isfinite(a[-1][k]).all() for k in keys)


@pytest.mark.parametrize("case", sorted(_CASES))
def test_deterministic_mode_agrees_with_the_default_build_step_by_step(case):
    """One EM step from the same parameters in both builds, over a short trajectory: the quantum costs at most the rounding
    error the plain sums make on their largest entries (1e-9 here; a lost or doubled atomic update would be orders above)."""
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU box (MI355X)")
    fn, shape = _CASES[case]
    make, p0, y, keys = fn(shape)
    md, mp = make(), make()
    md.deterministic = True
    p = _copy(p0)
    for it in range(8):
        an = _An(T=1.3 if it < 3 else 1.0, Ncut_factor=0.5 if (it >= 6 and not case.startswith("gsc")) else 0.0)
        qd = md.step(an, _copy(p), {"y": y})
        qp = mp.step(an, _copy(p), {"y": y})
        for k in keys:
            ref = np.asarray(qp[k], dtype=np.float64)
            got = np.asarray(qd[k], dtype=np.float64)
            if case.startswith("mca") and k == "W":
                # W_new = Wp / Wq element by element: where both are a few quanta the ratio is ill-determined in either build
                # (a quantum is 2^-52 of the bound N on Wq: an element whose Wq is 1e-6 keeps seven digits)
                rel = np.abs(got - ref) / (np.abs(ref) + 1e-300)
                assert (rel <= 1e-7).mean() > 0.95 and np.median(rel) < 1e-11, \
                    "%s step %d: %d elements of W apart, median %.2e" % (case, it, int((rel > 1e-7).sum()), np.median(rel))
                continue
            np.testing.assert_allclose(got, ref, rtol=1e-8, atol=1e-9 * max(1.0, float(np.abs(ref).max())),
                                       err_msg="%s step %d %s" % (case, it, k))
        p = {k: qp[k] for k in qp}


def test_default_build_is_not_bitwise_reproducible_where_the_deterministic_one_is():
    """What the mode is for: the same loop in the DEFAULT build at a size where many atomics race (BSC, 20k datapoints) --
    two runs are expected to differ in the last bits somewhere (reported, not required: nothing forces a race to show), the
    deterministic build's two runs may not."""
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU box (MI355X)")
    make, p0, y, keys = _bsc((64, 160, 8, 3, 20000))
    sched = lambda it: {"T": 1.0}
    runs = {det: [_loop(make, p0, y, keys, 12, det, sched) for _ in range(2)] for det in (False, True)}
    differing = {det: sum(any(not np.array_equal(a[k], b[k]) for k in keys) for a, b in zip(*runs[det])) for det in runs}
    print("steps (of 12) whose parameters differ between two identical runs: default build %d, deterministic build %d"
          % (differing[False], differing[True]))
    assert differing[True] == 0
    for a, b in zip(runs[False][0], runs[True][0]):          # ... and the two builds stay within rounding of each other
        for k in keys:
            np.testing.assert_allclose(b[k], a[k], rtol=1e-7, atol=1e-9 * max(1.0, float(np.abs(a[k]).max())))


def _gsc_big(N=30000, D=256, H=128):
    """Config-4 dimensions at a size where the list pass has dense rows for the gathered GEMM (vectorised generator)."""
    from prosper_amd.em.camodels.gsc_et import GSC
    rng = np.random.RandomState(15)
    W = rng.normal(size=(D, H))
    s = rng.uniform(size=(N, H)) < 2.0 / H
    z = s * (1.5 + rng.normal(size=(N, H)))
    y = z @ W.T + rng.normal(size=(N, D))
    p = {"W": W + 0.1 * rng.normal(size=(D, H)), "pi": np.full(H, 2.2 / H), "mu": np.full(H, 1.4),
         "psi_sq": np.eye(H) * 1.1, "sigma_sq": 1.2}
    return (lambda: GSC(D, H, 6, 3, "scalar")), p, y, ("W", "pi", "mu", "psi_sq", "sigma_sq")


def test_gsc_deterministic_mode_keeps_the_speculated_list_pass():
    """Round 6: the deterministic mode no longer switches off what makes GSC's EM loop fast -- the M-step launches the next
    E-step (quanta derived on the device from the parameters it has just solved: pm_gsc_det_quanta_f64), that pass writes
    lists, and its dense rows go through the gathered GEMM in ascending order (pm_sort_row_list_i32).  Two runs: identical
    bits at every step; the passes are adopted; and the loop stays within rounding of the default build's."""
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU box (MI355X)")
    make, p0, y, keys = _gsc_big()
    yd = torch.from_numpy(y).cuda()
    hits = []

    def loop(det, steps=14):
        m = make()
        m.deterministic = det
        p, traj = _copy(p0), []
        for it in range(steps):
            p = m.step(_An(T=1.2 if it < 4 else 1.0), p, {"y": yd})
            traj.append({k: np.array(p[k], copy=True) for k in keys})
        hits.append(m.spec_hits)
        return traj

    a, b, c = loop(True), loop(True), loop(False)
    assert hits[0] >= 10 and hits[0] == hits[1], hits            # (the temperature moves once: one dropped pass)
    for it, (pa, pb) in enumerate(zip(a, b)):
        for k in keys:
            assert np.array_equal(pa[k], pb[k]), "step %d, %s differs between two deterministic runs" % (it, k)
    for k in keys:       # same trajectory as the default build up to the quanta (14 steps of error growth: loose)
        np.testing.assert_allclose(a[-1][k], c[-1][k], rtol=1e-6, atol=1e-8 * max(1.0, float(np.abs(c[-1][k]).max())))


def test_sort_row_list_and_device_quanta():
    """pm_sort_row_list_i32 against np.sort on a shuffled list; pm_gsc_det_quanta_f64 against GSC._det_quanta's host bounds."""
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU box (MI355X)")
    import ctypes
    from prosper_amd import _lib
    rng = np.random.RandomState(5)
    for N, cnt in ((1000, 0), (1000, 1), (1000, 1000), (1003, 1003), (200_000, 41_237), (1 << 20, 77_777), (3_000_001, 500_000)):
        rows = rng.permutation(N)[:cnt].astype(np.int32)
        buf = torch.full((max(cnt, 1) + 8,), -7, dtype=torch.int32, device="cuda")
        buf[:cnt] = torch.from_numpy(rows).cuda()
        count = torch.tensor([cnt], dtype=torch.int32, device="cuda")
        nflag = (N + 7) // 8 * 8
        flags = torch.zeros(nflag + 4 * ((N + 8191) // 8192), dtype=torch.uint8, device="cuda")
        _lib.call("pm_sort_row_list_i32", ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(count.data_ptr()), N,
                  ctypes.c_void_p(flags.data_ptr()), None)
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert np.array_equal(got[:cnt], np.sort(rows)) and (got[cnt:] == -7).all(), (N, cnt)
        assert int(flags[:nflag].sum()) == 0, "the flag array is handed back cleared"
    make, p, y, _ = _gsc((128, 128, 6, 3, 600))
    m = make()
    m.deterministic = True
    res = m._resident(y)
    par = m._tables_for(p, res)
    from prosper_amd.em.camodels import _device
    _device._DET_QUANTA_SET.clear()
    m._det_quanta(res, p)
    host = _device._DET_QUANTA_SET["gsc"][:3] + _device._DET_QUANTA_SET["gemm"][:1]
    H = m.H
    tab = torch.zeros(9 * H, dtype=torch.float64, device="cuda")
    tab[:8 * H] = par["tables"].reshape(-1)[:8 * H]
    tab[8 * H] = 1.0 / par["s2"]
    made = m._det_dev_quanta(res, par["G"], par["psi_d"], tab)
    torch.cuda.synchronize()
    q = made["q"].cpu().numpy()
    assert tuple(q[:3]) + (q[8],) == host, (q, host)
    assert all(_device._DET_QUANTA_SET[u] is made for u in ("gsc", "gemm", "wp_sparse"))
