"""tests/gsc_kernels_reference.py pinned without a device: its statements of GSC's selection, log-joints, expectations and
statistics against oracle/gsc_oracle.py (component_scores, select_hprimes, compute_lpj, e_step) at small well-conditioned
shapes, to 1e-12 relative, with the tables built the way GSC._tables_for builds them; the dispatch table of
tests/test_gsc_kernels_gpu.py against pm_gsc_plan (a host-only query: the launchers switch on the same function); and the
properties of that module's data its comparisons rest on.

Cells of pm_gsc_plan(PM_GSC_PLAN_ESTEP), swept over H <= 512, H' <= 16, gamma <= 8 with the full state table of (H', gamma):
all 6 x 5 x 3 = 90 (VPL, GMAX, form) cells of the statistics / log-joint forms are reachable, none is listed as unreachable.
Two families are reachable only in a degenerate way, and their cases say so: VPL = 32 with the LACC form needs H <= 297 and
H' = 1 (20 H doubles of tables and accumulators leave no room for more), so those five cells have no multi-cause state
whatever GMAX is instantiated; the plain form at VPL <= 2 needs H' = 10 (H' = 9 there still fits the LACC layout, H' = 11
exceeds 64 KB).  With the four LIST cells the table holds 94 cells; the list-pairs cells are H = 64, 128, 192, 256."""
import ctypes
import functools
import itertools

import numpy as np
import pytest

import gsc_kernels_reference as R
from oracle import gsc_oracle as GO

PM_OK, PM_EINVAL, PM_ERANGE = 0, -1, -2
RTOL = 1e-12
LD = np.longdouble
ALL = list(R.ALL_CASES)


def _lib():
    from prosper_amd import _lib
    return _lib.load()


def _plan(which, H, Hp, S, gamma, D, flags, N, cus=0):
    out = (ctypes.c_int32 * R.PLAN_LEN)(*([-7] * R.PLAN_LEN))
    rc = _lib().pm_gsc_plan(which, H, Hp, S, gamma, D, flags, N, cus, out)
    return rc, tuple(out)


def _close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale = np.abs(want).max() if want.size else 1.0
    assert np.abs(got - want).max() <= RTOL * max(scale, 1e-300), (what, float(np.abs(got - want).max()), float(scale))


@functools.lru_cache(maxsize=None)
def _case(name, hot):
    c = R.make_case(name, hot)
    cand = R.select(c)
    return c, cand, R.estep(c, cand)


# ------------------------------------------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("D,H,Hp,gamma,T,sym", [(9, 6, 3, 2, 1.0, True), (8, 7, 4, 3, 1.3, False), (10, 5, 5, 5, 1.1, False),
                                                (6, 4, 2, 1, 1.0, True), (12, 9, 1, 3, 1.2, False)])
def test_reference_matches_the_gsc_oracle(D, H, Hp, gamma, T, sym):
    rng = np.random.RandomState(10 * D + H)
    model = GO.make_model(D, H, Hp, gamma)
    N = 21
    W = rng.normal(size=(D, H))
    psi = np.diag(rng.uniform(0.7, 1.4, size=H)) + 0.05 * rng.uniform(-1, 1, size=(H, H)) * (1 - np.eye(H))
    if sym:
        psi = 0.5 * (psi + psi.T)
    params = dict(W=W, mu=rng.uniform(-0.6, 0.6, size=H), psi_sq=psi, pi=rng.uniform(0.1, 0.5, size=H), sigma_sq=0.8)
    Y = rng.normal(size=(N, D)) * 1.3
    SM = model['SM'].astype(np.int64)
    masks = (SM << np.arange(SM.shape[1])[None, :]).sum(axis=1).astype(np.uint16) if SM.size else np.zeros(0, np.uint16)
    gram = W.T @ W
    c = dict(H=H, Hp=model['Hprime'], gamma=model['gamma'], S=len(masks), N=N, masks=masks, scores=Y @ W, gram=gram, psi_sq=psi,
             ynorm2=(Y * Y).sum(axis=1), sigma_sq=0.8, beta=1.0 / T,
             tables=R.make_tables((W * W).sum(axis=0), np.diag(psi), params['mu'], params['pi'], 0.8))
    if len(masks):
        assert np.array_equal(masks, R.state_masks(c["Hp"], c["gamma"])), "the table order of generate_state_matrix"
    _close(R.component_scores(c), GO.component_scores(params, Y), "component scores")
    cand = GO.select_hprimes(params, Y, c["Hp"])
    assert np.array_equal(R.select(c), cand)
    e = R.estep(c, cand)
    _close(e["lp"], GO.compute_lpj(model, params, Y, cand), "logpj")
    want = GO.e_step({'T': T}, model, params, Y, cand)
    _close(e["xpt_s"], want['xpt_s'], "xpt_s")
    _close(e["xpt_sz"], want['xpt_sz'], "xpt_sz")
    yy = float(c["ynorm2"].sum())
    for lacc in (False, True):
        packed = R.packed_stats(R.raw_stats(c, e, lacc), H, yy)
        sec = R.sections(H, packed=True)
        _close(packed[sec["ss"]].reshape(H, H), want['xpt_ss'].sum(axis=0), "sum xpt_ss")
        _close(packed[sec["zz"]].reshape(H, H), want['xpt_szsz'].sum(axis=0), "sum xpt_szsz")
        _close(packed[sec["s"]], want['xpt_s'].sum(axis=0), "sum xpt_s")
        _close(packed[sec["sz"]], want['xpt_sz'].sum(axis=0), "sum xpt_sz")
    # the blocks of compute_posterior_hprime: un-normalised sums over the multi-cause states, in `cand` order
    HH = c["Hp"] ** 2
    if len(masks):
        ss = np.zeros((N, c["Hp"], c["Hp"]))
        for s in range(len(masks)):
            pos = list(R.mask_positions(masks[s]))
            lp, _, _, idx = GO._state_quantities(params, Y, cand, tuple(pos))
            lpi = np.log(params['pi']) - np.log(1 - params['pi'])
            p = np.maximum(np.exp((lp + lpi[idx].sum(axis=1)) / T), R.TINY)
            ss[np.ix_(range(N), pos, pos)] += p[:, None, None]
        _close(e["blocks"][:, :HH], ss.reshape(N, HH), "blocks: sum p [i, k in s]")
        _close(e["blocks"][:, -1], ss[:, 0, 0] * 0 + e["w"][:, 1 + H:].sum(axis=1), "blocks: sum p")
    # the lists and their products
    idx, vz, vs, written, dense, nsig = R.list_split(e["xpt_s"], e["xpt_sz"], 0.0)
    assert (nsig == H).all() and len(dense) == 0 and H <= R.NZ_MAX
    pairs = R.list_pairs(idx, vs, vz, H).reshape(2, H, H)
    _close(pairs[0], want['xpt_s'].T @ want['xpt_sz'], "xs^T xsz")
    _close(pairs[1], want['xpt_sz'].T @ want['xpt_sz'], "xsz^T xsz")


# ---------------------------------------------------------------------------------------------------------- the plan
def test_plan_sweep_reaches_every_cell_and_the_table_holds_it():
    """Every (VPL, GMAX, form) the plan returns over H <= 512, H' <= 16, gamma <= 8 is a cell of the case table and vice versa;
    both ends of H of every VPL bucket appear among the cases."""
    lib = _lib()
    out = (ctypes.c_int32 * R.PLAN_LEN)()
    seen = set()
    for H in range(1, 513):
        for Hp in range(1, 17):
            for gamma in (1, 2, 3, 4, 5, 6, 7, 8):
                S = R.full_states(Hp, gamma)
                ok = bool(lib.pm_gsc_supported(H, Hp, gamma))
                for flags in (0, R.F_LPJ):
                    rc = lib.pm_gsc_plan(R.ESTEP, H, Hp, S, gamma, 0, flags, 37, 0, out)
                    assert rc == (PM_OK if ok else PM_ERANGE), (H, Hp, gamma, flags, rc)
                    if rc == PM_OK:
                        seen.add((out[0], out[1], out[2]))
                        vpl = 1 if H <= 16 else 2 if H <= 32 else 4 if H <= 64 else 8 if H <= 128 else 16 if H <= 256 else 32
                        gmax = 2 if gamma <= 2 else gamma if gamma <= 4 else 6 if gamma <= 6 else 8
                        assert (out[0], out[1]) == (vpl, gmax) and out[2] in ((R.LPJ,) if flags else (R.PLAIN, R.LACC))
                        assert out[6] == (out[2] != R.LACC) and out[4] == 3 and out[5] == 1
    assert len(seen) == 90
    table = {R.case_shape(n)["cell"] for n in R.CASES}
    assert {cl for cl in table if cl[2] != R.LIST} == seen
    assert {cl for cl in table if cl[2] == R.LIST} == {(8, 2, R.LIST), (8, 3, R.LIST), (16, 2, R.LIST), (16, 3, R.LIST)}
    hs = {R.case_shape(n)["H"] for n in R.CASES}
    assert {1, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512} <= hs


@pytest.mark.parametrize("name", ALL)
def test_case_cells(name):
    """pm_gsc_plan of every case equals its literal cell; LDS, grid, trips and the colsum flag follow from the documented
    formulas."""
    c = R.case_shape(name)
    rc, p = _plan(R.ESTEP, c["H"], c["Hp"], c["S"], c["gamma"], 0, c["flags"], c["N"], 256)
    assert rc == PM_OK and p[:3] == c["cell"], (name, rc, p)
    base = 8 * (8 * c["H"] + 16 * (48 + 4 * c["Hp"] ** 2) + (c["S"] + 3) // 4)
    lacc = base + 8 * (12 * c["H"] + 1)
    assert p[3] == (lacc if lacc <= 53 * 1024 else base), (name, p)
    if c["cell"][2] in (R.LACC, R.LIST):
        assert lacc <= 53 * 1024
    if c["cell"][2] == R.PLAIN:
        assert lacc > 53 * 1024
    assert p[4] == -(-c["N"] // 16) and p[5] == 1 and p[6] == int(c["cell"][2] in (R.PLAIN, R.LPJ)) and p[7:] == (0,) * 5
    assert 16 < c["N"] < 64 and c["N"] % 16 != 0
    if c["flags"] & R.F_LPJ:
        rc, pb = _plan(R.ESTEP, c["H"], c["Hp"], c["S"], c["gamma"], 0, R.F_LPJ | R.F_BLOCKS, c["N"], 256)
        assert rc == PM_OK and pb == p


def test_plan_grid_and_trips():
    """The grid is capped at three workgroups per CU (`cus <= 0`: 256), the trips follow; the LIST floor ceil(N / 512) binds
    from N = 512 * 3 * cus + 1 on (pinned here, never launched)."""
    for cus, eff in ((0, 256), (-3, 256), (256, 256), (304, 304), (8, 8)):
        cap = 3 * eff
        for N, grid, trips in ((1, 1, 1), (16, 1, 1), (17, 2, 1), (16 * cap, cap, 1), (16 * cap + 1, cap, 2),
                               (16 * (cap + 3) + 5, cap, 2), (32 * cap + 1, cap, 3)):
            for flags, H in ((0, 12), (R.F_LPJ, 12), (R.F_LISTS, 128)):
                if flags == R.F_LISTS and N > 512 * cap:
                    continue
                rc, p = _plan(R.ESTEP, H, 3, 3, 2, 0, flags, N, cus)
                assert rc == PM_OK and p[4:6] == (grid, trips), (cus, N, flags, p)
        N = 512 * cap + 1
        rc, p = _plan(R.ESTEP, 128, 3, 3, 2, 0, R.F_LISTS, N, cus)
        assert rc == PM_OK and p[4] == cap + 1 and p[5] == -(-(-(-N // 16)) // (cap + 1)) and p[5] <= 32, (cus, p)
        rc, p = _plan(R.ESTEP, 128, 3, 3, 2, 0, R.F_LISTS, N - 1, cus)
        assert rc == PM_OK and p[4] == cap and p[5] == 32, (cus, p)
        rc, p = _plan(R.ESTEP, 128, 3, 3, 2, 0, 0, N, cus)
        assert rc == PM_OK and p[4] == cap and p[5] == 33, (cus, p)


def test_plan_lists_and_lists_supported_agree():
    """pm_gsc_lists_supported is the plan with LISTS, the full table and D > 0."""
    lib = _lib()
    for H, Hp, gamma, D in itertools.product((64, 65, 128, 192, 256, 257, 384), (1, 4, 8, 9, 12), (1, 2, 3, 4), (0, 100, 128, 256, 1024)):
        S = R.full_states(Hp, gamma)
        rc, _ = _plan(R.ESTEP, H, Hp, S, gamma, D, R.F_LISTS, 100)
        assert bool(lib.pm_gsc_lists_supported(H, Hp, gamma, D)) == (rc == PM_OK and D > 0), (H, Hp, gamma, D, rc)
        want = bool(lib.pm_gsc_supported(H, Hp, gamma)) and gamma <= 3 and 64 < H <= 256 \
            and 8 * (20 * H + 16 * (48 + 4 * Hp * Hp) + (S + 3) // 4 + 1) <= 53 * 1024 \
            and (D <= 0 or ((D + 2 * H) % 128 == 0 and H % 128 == 0))
        assert (rc == PM_OK) == want, (H, Hp, gamma, D, rc)


@pytest.mark.parametrize("H", sorted(R.LIST_PAIRS_CELLS))
def test_list_pairs_cells(H):
    """rows_c is the largest divisor of H with rows_c * H <= 16384: 64, 128 and 256 keep the values they had (H, H, 64), and 192
    gets 64 in three chunks."""
    rc, p = _plan(R.LIST_PAIRS, H, 0, 0, 0, 0, 0, 45)
    assert rc == PM_OK and p[7:11] == R.LIST_PAIRS_CELLS[H] and p[:3] == (0, 0, 0), p
    rows_c = p[7]
    assert H % rows_c == 0 and rows_c * H <= 16384 and all(H % r or r * H > 16384 for r in range(rows_c + 1, H + 1))
    assert p[3] == 8 * rows_c * H and p[4] == 2 * p[8] * p[9]
    old = {64: 64, 128: 128, 256: 64}
    assert H == 192 or rows_c == old[H]
    # many datapoints: 256 / (2 nchunks) groups of a multiple of 64 datapoints
    rc, p = _plan(R.LIST_PAIRS, H, 0, 0, 0, 0, 0, 200000)
    groups = 256 // (2 * p[8])
    rpg = -(-(-(-200000 // groups)) // 64) * 64
    assert rc == PM_OK and p[10] == rpg and p[9] == -(-200000 // rpg) and p[5] == -(-rpg // 512)


def test_pack_and_component_scores_plans():
    assert _plan(R.PACK, 512, 0, 0, 0, 0, 0, 1)[1][4] == 1024 and _plan(R.PACK, 1, 0, 0, 0, 0, 0, 1)[1][4] == 1
    assert _plan(R.COMPONENT_SCORES, 7, 0, 0, 0, 0, 0, 37)[1][4] == 2
    assert _plan(R.COMPONENT_SCORES, 512, 0, 0, 0, 0, 0, (2 ** 31 - 1) // 2)[0] == PM_OK


@pytest.mark.parametrize("k", range(len(R.REFUSALS)))
def test_plan_refusals(k):
    (which, H, Hp, S, gamma, D, flags, N), want = R.REFUSALS[k]
    S = R.full_states(Hp, gamma) if S is None else S
    rc, p = _plan(which, H, Hp, S, gamma, D, flags, N)
    assert rc == want and p == (-7,) * R.PLAN_LEN, (R.REFUSALS[k], rc, p)
    assert _lib().pm_gsc_plan(R.ESTEP, 8, 2, 1, 2, 0, 0, 16, 0, None) == PM_EINVAL


# ---------------------------------------------------------------------------------------------- properties of the data
@pytest.mark.parametrize("name", ALL)
def test_hot_rows_are_flat(name):
    """HOT: all K = 1 + H + S weights of a row lie within a factor e."""
    c, cand, e = _case(name, True)
    x = LD(c["beta"]) * e["lp"]
    assert float((x.max(axis=1) - x.min(axis=1)).max()) <= 1.0, (name, float((x.max(axis=1) - x.min(axis=1)).max()))
    assert 1 < c["beta"] <= 2 and (c["tables"][7] == 0).all()


@pytest.mark.parametrize("name", ALL)
def test_cold_rows_sit_on_the_clamp(name):
    """COLD: states on both sides of log(tiny), an argument inside the libm window, and a row in which every state, the null
    state included, underflows."""
    c, cand, e = _case(name, False)
    x = np.asarray(LD(c["beta"]) * e["lp"], dtype=np.float64)
    assert (x < R.LOG_TINY - 1e-6).any() and (x > R.LOG_TINY + 1e-6).any(), name
    assert ((x[:, 1:] >= R.LOG_TINY + 1e-9) & (x[:, 1:] < R.WINDOW_HI - 1e-9)).any(), name
    under = (x < R.LOG_TINY - 1e-6).all(axis=1)
    assert under.any(), name
    K = x.shape[1]
    r = int(np.argmax(under))
    assert abs(float(e["Z"][r]) / ((K - 1) * R.TINY) - 1) < 1.0 / (K - 1) + 1e-12, "Z = K tiny (the null state is not clamped)"
    mixed = ((x < R.LOG_TINY).any(axis=1) & (x > R.LOG_TINY).any(axis=1))
    assert mixed.any(), name


@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("hot", [True, False])
def test_conditioning_cap(name, hot):
    """Every state's Psi_a and Lambda_a -- with the full table every 2..gamma-subset of a row's candidates -- has a condition
    number of at most 16: the kernel's unpivoted Gauss-Jordan is well inside the bound.  The selection's cut is clear:
    the H'-th and (H'+1)-th scores differ by more than 2^-30 relative, far above the 10 mantissa bits the ranking drops."""
    c, cand, e = _case(name, hot)
    worst = 0.0
    for s in range(c["S"]):
        _, _, _, _, P, Lam = R.state_terms(c, cand, R.mask_positions(c["masks"][s]))
        worst = max(worst, float(np.linalg.cond(P.astype(np.float64)).max()), float(np.linalg.cond(Lam.astype(np.float64)).max()))
    assert worst <= 16.0, (name, worst)
    assert (R.selection_gap(c) > 2.0 ** -30).all(), name
    assert (np.diff(cand, axis=1) > 0).all() and cand.min() >= 0 and cand.max() < c["H"]


SELECTION_SHAPES = [(1, 1), (16, 3), (17, 10), (32, 5), (33, 2), (64, 9), (65, 10), (128, 7), (129, 3), (256, 9), (257, 4),
                    (512, 6)]


@pytest.mark.parametrize("H,Hp", SELECTION_SHAPES)
def test_selection_scores_are_exact(H, Hp):
    """The finite scores of the selection cases have at most 43 significant bits (the ranking drops none of them), the same
    value in float64 and longdouble arithmetic, real ties at the cut and inside the selected set, and the edge rows hold what
    they are meant to."""
    c = R.make_selection_case(H, Hp)
    v = R.component_scores(c, clamp=False)
    fin = np.isfinite(v)
    assert np.array_equal(R.rank_values(v[fin]), v[fin])
    t, a, yn = c["tables"], c["scores"], c["ynorm2"]
    with np.errstate(invalid="ignore", over="ignore"):
        b = a - t[2][None, :]
        v64 = t[0][None, :] - yn[:, None] * 0.25 + t[1][None, :] * a + b * b * t[3][None, :]
    assert np.array_equal(v64[fin], v[fin])
    assert (v[9] == np.inf).any() and (H == 1 or (v[9][np.isfinite(v[9])] < 0).sum() >= 1) and np.isnan(v[10]).any()
    assert (v[11] == -np.inf).all() and np.isnan(v[12]).all()
    vc = R.component_scores(c)
    assert (vc[11] == -R.DBL_MAX).all() and (vc[12] == -R.DBL_MAX).all() and (vc[9][v[9] == np.inf] == 0).all()
    assert (vc[10][np.isnan(v[10])] == -R.DBL_MAX).all()
    cand = R.select(c)
    if H > Hp:
        tie_cut = tie_in = 0
        for n in range(8):
            s = np.sort(vc[n])
            tie_cut += s[H - Hp] == s[H - Hp - 1]
            tie_in += Hp > 1 and (np.diff(s[H - Hp:]) == 0).any()
        assert tie_cut >= 1 and (Hp == 1 or tie_in >= 1), (H, Hp)
        assert np.array_equal(cand[11], np.arange(H - Hp, H)) and np.array_equal(cand[12], np.arange(H - Hp, H))
    for neg in (False, True):
        z = R.make_zero_case(H, Hp, neg)
        vz = R.component_scores(z, clamp=False)
        assert (vz == 0).all() and (np.signbit(vz) == neg).all()
        assert np.array_equal(R.select(z), np.tile(np.arange(H - Hp, H), (3, 1)))


@pytest.mark.parametrize("name", R.THRESHOLD_CASES)
@pytest.mark.parametrize("hot", [True, False])
def test_thresholds_are_clear_of_every_value(name, hot):
    """thr_p of the threshold cases drops some entries, keeps others, and no reference value lies within 1 +- 2^-20 of it."""
    c, cand, e = _case(name, hot)
    thr_p = R.pick_thr_p(e)
    v = R.pair_values(e)
    assert R.clear_of(thr_p, v) and (v > thr_p).any() and ((v < thr_p) & (v > 0)).any(), (name, thr_p)


@pytest.mark.parametrize("name", [n for n in R.CASES if R.CASES[n][6][2] == R.LIST])
@pytest.mark.parametrize("hot", [True, False])
def test_list_thresholds_are_clear_of_every_value(name, hot):
    c, cand, e = _case(name, hot)
    m = R.list_measure(e["xpt_s"], e["xpt_sz"])
    for k in (0, 1, 16, 17):
        row, thr = R.thr_for_count(e["xpt_s"], e["xpt_sz"], k)
        assert R.clear_of(thr, m), (name, k)
        assert R.list_split(e["xpt_s"], e["xpt_sz"], thr)[5][row] == k
