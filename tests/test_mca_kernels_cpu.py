"""tests/mca_kernels_reference.py pinned on the CPU: against oracle/mca_oracle.py and oracle/mmca_oracle.py at small shapes,
and the conditions a GPU test of these cases relies on, for every case of the table (pm_mca_plan is a host-only query:
the dispatch cells are confirmed here without a GPU).

Bound against the oracles.  The oracles are float64 NumPy: a log-joint is a sum of D squared differences, each from one exp
and one log (<= 1 ulp each, amplified by 1 / rho <= 1 and by rho log|W| <= 21 * 0.7 in the tables), times pre1, plus the
prior: relative to the row's largest |f| the rounding stays below (D + 40) u, u = 2^-53; the statistics add N (1 + H + S)
weighted terms, each with exp(beta f - max) whose argument carries |beta f| u <= 1500 u of absolute error.  With D <= 20,
N <= 12 and 1 + H + S <= 40 that is below 2e-13 relative to a section's largest entry; the tests use 1e-12."""
import ctypes

import numpy as np
import pytest

import mca_kernels_reference as R
from oracle import mca_oracle as MO
from oracle import mmca_oracle as MMO

LD = np.longdouble
PM_OK, PM_EINVAL, PM_ERANGE = 0, -1, -2
ORACLE_RTOL = 1e-12


def _lib():
    from prosper_amd import _lib
    return _lib.load()


def plan(which, c, N=None, defer=0, lib=None, **over):
    d = dict(H=c["H"], D=c["D"], Hp=c["Hp"], S=c["S"])
    d.update(over)
    out = (ctypes.c_int32 * R.PLAN_LEN)(*([-7] * R.PLAN_LEN))
    rc = (lib or _lib()).pm_mca_plan(which, d["H"], d["D"], d["Hp"], d["S"], int(c["signed"]), c["inv_rho"],
                                     c["N"] if N is None else N, defer, out)
    return rc, tuple(out)


def cell_of(which, p):
    """The part of a plan that names the instantiation."""
    return p[:4] + (p[7:10] if which == R.MSTEP_ROWS else ())


# ------------------------------------------------------------------------------------------------ against the oracles
def _oracle_case(signed, D, H, Hp, gamma, N, T, seed):
    O = MMO if signed else MO
    rng = np.random.RandomState(seed)
    W = rng.uniform(0.4, 1.8, size=(D, H)) * (rng.choice([-1.0, 1.0], size=(D, H)) if signed else 1.0)
    Y = rng.uniform(0.0, 2.0, size=(N, D))
    model = O.make_model(D, H, Hp, gamma)
    cand = np.stack([rng.permutation(H)[:Hp] for _ in range(N)]).astype(np.int64)
    pies, sigma = 0.2, 0.9
    anneal = O.Anneal(T=T, Ncut_factor=0.0)
    rho = float(O.rho_of(T))
    wrho, wrm1, wn = R.tables(W.T, rho, signed)
    masks = np.array([sum(1 << j for j in np.nonzero(row)[0]) for row in model["SM"]], dtype=np.uint16)
    c = dict(H=H, D=D, Hp=Hp, S=len(masks), N=N, rows=N, signed=signed, inv_rho=1.0 / rho, beta=1.0 / T, Y=Y,
             cand=cand.astype(np.int32), masks=masks, Wrho=wrho, Wrm1=wrm1, wnorm2=wn, ynorm2=(Y * Y).sum(axis=1),
             scores=Y @ W, pil_bar=float(np.log(pies / (1 - pies))), pre1=-0.5 / sigma ** 2)
    F_o = O.e_step_vec(anneal, W, pies, sigma, Y, cand, model["SM"], model["state_abs"])
    _, log = O.m_step(anneal, model, W, pies, sigma, Y, cand, F_o, vec=True)
    return c, W, F_o, log["stats"], O


@pytest.mark.parametrize("signed", [0, 1])
@pytest.mark.parametrize("shape", [(5, 4, 3, 2, 7, 1.0), (20, 6, 4, 3, 12, 1.3), (9, 7, 5, 4, 5, 1.2), (3, 3, 2, 2, 4, 2.0)])
def test_reference_matches_oracle(signed, shape):
    D, H, Hp, gamma, N, T = shape
    c, W, F_o, st, O = _oracle_case(signed, D, H, Hp, gamma, N, T, seed=D + H)
    Y = c["Y"]
    F = R.logpj(c)
    scale = np.abs(F_o).max(axis=1, keepdims=True)
    assert (np.abs(F.astype(np.float64) - F_o) <= ORACLE_RTOL * scale).all()
    l1, lb = R.lse(F, c["beta"])
    assert np.allclose(l1.astype(np.float64), np.log(np.exp(F_o).sum(axis=1)), rtol=ORACLE_RTOL, atol=0)
    corr = c["beta"] * F_o.max(axis=1)                      # the oracle's stabilised log-denominators (mca_et.py:250-258)
    denoms = np.log(np.exp(c["beta"] * F_o - corr[:, None]).sum(axis=1)) + corr
    assert (np.abs(lb.astype(np.float64) - denoms) <= ORACLE_RTOL * np.abs(c["beta"] * F_o).max(axis=1)).all()
    add, q1, _ = R.packed_stats(c, F, l1, lb, np.ones(N, dtype=bool))
    HD = H * D
    G1 = (q1.T @ Y.astype(LD)).reshape(-1)
    w2 = ((W.T * W.T).reshape(-1) if not signed else np.ones(HD)).astype(LD)
    Wp = (G1 * w2 + add[HD:2 * HD]).astype(np.float64).reshape(H, D)
    Wq = (np.repeat(add[3 * HD:3 * HD + H], D) * w2 + add[2 * HD:3 * HD]).astype(np.float64).reshape(H, D)
    for got, want in ((Wp, st["Wp"]), (Wq, st["Wq"])):
        assert np.abs(got - want).max() <= ORACLE_RTOL * np.abs(want).max()
    o = 3 * HD + H
    assert abs(float(add[o]) - st["pi"]) <= ORACLE_RTOL * abs(st["pi"])
    assert abs(float(add[o + 1]) - st["sigma"]) <= ORACLE_RTOL * abs(st["sigma"])
    assert float(add[o + 3]) == N
    # the W update on these statistics is the oracle's (float64 on both sides: a few ulp).  pm_mca_w_update_f64 is the MCA
    # update G1 W^2 + Wp_m over q1sum W^2 + Wq_m (mca_et.py:333-348); MMCA's has no W^2 and is not that entry point's
    stats = np.concatenate([G1.astype(np.float64), add[HD:].astype(np.float64)])
    if not signed:
        new, clamped = R.w_update(stats, W.T, H, D, 1e-4)
        assert np.allclose(new, st["Wp"] / st["Wq"], rtol=1e-11, atol=0)
        assert np.array_equal(clamped, np.maximum(new, 1e-4))
    # the deferred records are the same statistics, datapoint by datapoint
    rec, sc = R.defer_records(c, F, l1, lb)
    add2, _, keep = R.defer_apply(H, D, lb, -np.inf, Y, c["cand"], rec, sc, q1)
    assert keep.all() and np.abs(add2 - add).max() <= 1e-17 * np.abs(add).max() + 1e-300


def test_select_scores_reference():
    rng = np.random.RandomState(3)
    W, Y = rng.uniform(0, 2, size=(6, 5)), rng.uniform(0, 2, size=(8, 6))
    assert np.allclose(R.select_scores(Y, W.T).astype(np.float64), MO.select_scores_vec(W, Y), rtol=1e-14)


# ----------------------------------------------------------------------------------------------- the table of cases
@pytest.mark.parametrize("name", list(R.CASES))
def test_case_cells(name):
    """Every case lands in the instantiation it is meant for."""
    c = R.make_case(name, True)
    for which, want in c["cells"].items():
        rc, p = plan(which, c)
        if want is None:
            assert rc == PM_ERANGE, (name, which, rc, p)
        else:
            assert rc == PM_OK and cell_of(which, p) == want, (name, which, rc, p)
    if c["N"] > 8192:
        for which in c["cells"]:
            assert plan(which, c)[1][6] == 2048, "the grid is the cap: a wavefront takes a second datapoint"
        assert plan(R.DEFER_APPLY, c)[1][14] == 2048


def test_table_covers_every_cell():
    """The cells of CASES (pinned to pm_mca_plan by test_case_cells) are ALL the instantiations the launchers can pick: the ten
    (DPL, HP) tiles of the fused pass with DPL HP <= 48, for unsigned W, signed W at rho = 6 and signed W at another rho; every
    (DPL, HP) of the two-pass M-step (DPL <= 8 at HP 4 / 8, <= 4 at HP 12, <= 2 at HP 16; a walk's last slab counts) for both
    signs; the five DPL of the E-step with its three powers; the paired form on exactly (12, 2), (8, 4), (12, 4) of signed W."""
    tiles = {(d, h) for d in (1, 2, 4, 8) for h in (4, 8, 12) if d * h <= 48}
    assert len(tiles) == 10
    fused, mstep, estep = set(), set(), set()
    for name, row in R.CASES.items():
        signed, cells = row[5], row[8]
        if cells[R.FUSED] is not None:
            d, h, root, paired = cells[R.FUSED]
            fused.add((d, h, "u" if not signed else "s6" if root == 6 else "s"))
            assert paired == (1 if signed and (h, d) in ((12, 2), (8, 4), (12, 4)) else 0), name
        d, h, _, _, _, _, last = cells[R.MSTEP_ROWS]
        mstep |= {(d, h, signed), (last, h, signed)}
        estep.add((cells[R.ESTEP][0], cells[R.ESTEP][2], signed))
    assert fused == {(d, h, k) for d, h in tiles for k in ("u", "s6", "s")}, sorted({(d, h, k) for d, h in tiles for k in ("u", "s6", "s")} - fused)
    want_m = {(d, h, sg) for sg in (0, 1) for h, dmax in ((4, 8), (8, 8), (12, 4), (16, 2)) for d in (1, 2, 4, 8) if d <= dmax}
    assert mstep == want_m, sorted(want_m - mstep)
    assert {d for d, _, _ in estep} == {1, 2, 4, 8, 16}
    assert {(r, sg) for _, r, sg in estep} == {(21, 0), (6, 0), (0, 0), (6, 1), (0, 1)}


@pytest.mark.parametrize("name", list(R.CASES))
def test_case_conditions(name):
    c = R.make_case(name, True)
    ref = R.case_reference(c)
    bf = c["beta"] * ref["F"]
    assert float((bf.max(axis=1) - bf.min(axis=1)).max()) < 1.0, "HOT: all weights of a row within a factor e"
    assert len(set(map(tuple, c["cand"][:c["rows"]]))) > 1 or c["H"] == c["Hp"]
    assert all(len(set(r)) == c["Hp"] for r in c["cand"][:c["rows"]]), "candidates of a datapoint are distinct"
    assert int(c["masks"].max(initial=0)) < (1 << c["Hp"])
    if c["kind"] == "odd":
        m = c["masks"]
        assert (np.array([bin(x).count("1") for x in m]) == 1).sum() >= 2 and m[-1] == m[1]
    cold = R.make_case(name, False)
    rc = R.case_reference(cold)
    assert R.exponent_conditioning(cold, rc["F"]) <= 2e-11, "float64 itself resolves the exponents of this case to 1e-11"
    d1 = rc["F"] - rc["F"].max(axis=1, keepdims=True)
    dall = cold["beta"] * rc["F"] - rc["lseb"][:, None]
    assert (d1 <= R.LSE_CUT).any(), "COLD: terms the log-evidence sums leave out"
    assert (dall < R.UNDERFLOW).any() and (dall > -1.0).any(), "COLD: weights that underflow to 0 beside weights that carry"
    if cold["S"]:
        dl = dall[:, 1 + cold["H"]:]
        assert (dl < R.QCUT).any() and (dl < R.UNDERFLOW).any(), "COLD: states below the cut-offs"
        assert (dl > -40.0).any(), "COLD: states that carry weight"
    if cold["S"] >= 20:
        assert ((dl > R.LSE_CUT) & (dl < -40.0)).any(), "COLD: states of tiny weight that must be kept"
    if name.startswith("s_zero"):
        for cc, rr in ((c, ref), (cold, rc)):
            t = R._tsum(cc, slice(0, cc["rows"]))
            assert (t == 0).any() and (t != 0).any(), "signed W with exact cancellations: t = 0 entries"
        # ... and in the COLD run a state WITH t = 0 entries whose weight underflows to exactly 0, beside one that carries
        zero_state = (R._tsum(cold, slice(0, cold["rows"])) == 0).any(axis=2)
        assert (zero_state & (dl < R.UNDERFLOW)).any() and (zero_state & (dl > -40.0)).any()


def test_cut_offs_are_told_apart():
    """The reference's three drop rules on log-joints placed in the narrow bands between them: -745 (log-evidence sums),
    -745.1332 (float64 underflow of exp) and -745.2 (`qcut` of the two-pass M-step)."""
    c = dict(H=1, Hp=2, S=4, beta=1.0, masks=np.array([3, 3, 3, 3], dtype=np.uint16), pil_bar=0.0, pre1=-1.0)
    F = np.array([[0.0, -800.0, -744.9, -745.05, -745.15, -745.3]])
    lb = np.zeros(1)
    q = R.posteriors(c, F, lb)[0, 2:]
    qc = R.posteriors(c, F, lb, R.QCUT)[0, 2:]
    assert (q[:2] > 0).all() and (q[2:] == 0).all(), "below -745.1332 a weight is exactly 0"
    assert np.array_equal(q, qc), "between -745.2 and -745.1332 a state is walked, with weight 0: no value changes"
    assert float(q[1].astype(np.float64)) == 5e-324, "between -745.1332 and -745 the weight is the smallest subnormal"
    # (a term at -745 of the maximum is e^-745 of the sum: leaving it out of the log-evidences changes no bit, in float64 or
    # in longdouble -- the rule is a saving, not a value)
    l1, _ = R.lse(F, 1.0)
    assert l1[0] == np.log(np.exp(F.astype(LD)).sum(axis=1))[0]


def test_plan_ranges_and_header_limits():
    """PM_ERANGE exactly where the launchers return it; the M-step's limits as prosper_hip.h states them: Hprime <= 16,
    slabs of 512 / 256 / 128 at Hprime <= 8 / <= 12 / <= 16."""
    from prosper_amd import _lib
    lib = _lib.load()
    assert lib.pm_version() >= 1024 and _lib.MIN_VERSION >= 1024
    c = dict(H=20, D=10, Hp=3, S=3, N=5, signed=0, inv_rho=1.0 / 21.0)
    out = (ctypes.c_int32 * R.PLAN_LEN)()
    assert lib.pm_mca_plan(0, 20, 10, 3, 3, 0, 0.1, 5, 0, None) == PM_EINVAL
    for bad in ((-1, 20, 10, 3, 3), (4, 20, 10, 3, 3), (0, 0, 10, 3, 3), (0, 20, 0, 3, 3), (0, 20, 10, 0, 3), (0, 20, 10, 3, -1)):
        assert lib.pm_mca_plan(*bad, 0, 0.1, 5, 0, out) == PM_EINVAL, bad
    assert lib.pm_mca_plan(0, 20, 10, 3, 3, 0, 0.1, 0, 0, out) == PM_EINVAL
    E, M, F, A = R.ESTEP, R.MSTEP_ROWS, R.FUSED, R.DEFER_APPLY
    for which, over in ((E, dict(D=1025)), (E, dict(Hp=17)), (E, dict(Hp=21)), (E, dict(S=65536)),
                        (M, dict(Hp=17)), (M, dict(Hp=21)), (M, dict(S=65536)), (M, dict(D=(1 << 20) + 1)),
                        (F, dict(D=513)), (F, dict(Hp=13)), (F, dict(D=257, Hp=5)), (F, dict(Hp=21, H=20)), (F, dict(S=65536)),
                        (A, dict(H=513)), (A, dict(D=513)), (A, dict(Hp=13))):
        assert plan(which, c, lib=lib, **over)[0] == PM_ERANGE, (which, over)
    for which, over in ((E, dict(D=1024, Hp=16)), (M, dict(Hp=16, D=1 << 20)), (F, dict(D=512, Hp=4)), (F, dict(D=256, Hp=12)),
                        (A, dict(H=512, D=512, Hp=12))):
        assert plan(which, c, lib=lib, **over)[0] == PM_OK, (which, over)
    for Hp, tile, slab in ((1, 4, 512), (4, 4, 512), (5, 8, 512), (8, 8, 512), (9, 12, 256), (12, 12, 256), (13, 16, 128),
                           (16, 16, 128)):
        for D, in ((1,), (slab,), (slab + 1,), (3 * slab + 65,)):
            rc, p = plan(M, c, lib=lib, Hp=Hp, D=D)
            last = D - (p[8] - 1) * slab
            assert rc == PM_OK and p[1] == tile and p[7] == slab and p[8] == -(-D // slab), (Hp, D, p)
            assert p[0] == min(slab, 64 * (1 if D <= 64 else 2 if D <= 128 else 4 if D <= 256 else 8)) // 64
            assert p[9] == (1 if last <= 64 else 2 if last <= 128 else 4 if last <= 256 else 8)
    # the fused pass: tiles, the pairs, the powers
    for Hp, D, sg, ir, want in ((4, 64, 0, 1 / 21, (1, 4, 0, 0)), (5, 64, 0, 1 / 21, (1, 8, 0, 0)), (9, 64, 1, 1 / 6, (1, 12, 6, 0)),
                                (9, 128, 1, 1 / 6, (2, 12, 6, 1)), (8, 256, 1, 0.3, (4, 8, 0, 1)), (12, 256, 1, 1 / 6, (4, 12, 6, 1)),
                                (8, 128, 1, 1 / 6, (2, 8, 6, 0)), (4, 512, 1, 1 / 6, (8, 4, 6, 0)), (12, 256, 0, 1 / 6, (4, 12, 0, 0))):
        cc = dict(c, signed=sg, inv_rho=ir)
        rc, p = plan(F, cc, lib=lib, Hp=Hp, D=D)
        assert rc == PM_OK and p[:4] == want, (Hp, D, sg, p)
        assert plan(F, cc, lib=lib, Hp=Hp, D=D, defer=1)[1][10] == 1
    # the deferred statistics: HR = 128 / 64 / 32 / 16 latent rows at DPL 1 / 2 / 4 / 8, groups of 256 datapoints up to 64
    for D, hr in ((64, 128), (65, 64), (129, 32), (257, 16)):
        for H, nr in ((hr, 1), (hr + 1, 2)):
            rc, p = plan(A, c, lib=lib, H=H, D=D, Hp=3)
            assert rc == PM_OK and (p[11], p[12]) == (min(hr, H), nr), (D, H, p)
    for N, G in ((1, 1), (255, 1), (256, 1), (257, 2), (1100, 5), (16200, 64), (65600, 64)):
        assert plan(A, c, lib=lib, N=N)[1][13] == G


@pytest.mark.parametrize("name", list(R.RESCALE))
def test_rescale_cases(name):
    """The `resc_*` cases really raise beta f_s by more than 50 over the lazily followed maximum at the intended states, on
    the intended tile (paired or not)."""
    base, sizes, points = R.RESCALE[name]
    c = R.make_rescale_case(name)
    ref = R.case_reference(c)
    assert R.rescale_points(c, ref) == points
    assert [bin(m).count("1") for m in c["masks"]] == list(sizes) and len(set(c["masks"].tolist())) == len(sizes)
    rc, p = plan(R.FUSED, c)
    assert rc == PM_OK and p[:4] == c["cells"][R.FUSED] and p[3] == (1 if name.startswith("resc_p") else 0)
    bf = c["beta"] * ref["F"][:, 1 + c["H"]:]
    for k in points[1:]:
        assert ((bf[:, k] - bf[:, :k].max(axis=1)) > 50).all()
