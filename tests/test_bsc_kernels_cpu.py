"""What runs without a device of the Binary Sparse Coding kernel tests: the dispatch of every launcher as pm_bsc_plan reports
it (a host-only query; the launchers, the *_supported predicates and pm_bsc_fused8_main_rows switch on the same functions), the
case table of tests/test_bsc_kernels_gpu.py against that plan and against the exactness its equality comparisons rest on, and
the NumPy reference tests/bsc_kernels_reference.py against oracle/bsc_oracle.py.

The dispatch, read from the launchers: pm_bsc_select_f64 VPL 1, 2, 4, 8, 16 at H <= 64, 128, 256, 512, 1024; the sixteen-lane
kernels VPL 1, 2, 4, 8, 16, 32 at H <= 16, 32, 64, 128, 256, 512; pm_bsc_estep_fused_f64 NJ 8 at H <= 128, 16 up to 256, FULL at
H = 16 NJ; pm_bsc_estep_fused8_f64 HP = H' in 5 .. 8, GAMMA 3 or 4, FULL at H = 256, the main launch for whole rounds of
cus 128 rows and for a ragged round of at least 70 % or of more than 2 cus 16 rows, the TAIL launch for the rest."""
import ctypes

import numpy as np
import pytest

import bsc_kernels_reference as R

PM_OK, PM_EINVAL, PM_ERANGE = 0, -1, -2
LD = np.longdouble


def _lib(det=False):
    from prosper_amd import _lib
    return _lib.load(det)


def plan(which, H, D, Hp, S, gamma, flags, N, cus=256, det=False):
    out = (ctypes.c_int32 * R.PLAN_LEN)(*([-7] * R.PLAN_LEN))
    rc = _lib(det).pm_bsc_plan(which, H, D, Hp, S, gamma, flags, N, cus, out)
    return rc, tuple(out)


def test_abi():
    from prosper_amd import _lib
    for path in (_lib.LIB_PATH, _lib.LIB_PATH_DET):
        assert hasattr(ctypes.CDLL(path), "pm_bsc_plan"), path
    assert _lib.load().pm_version() >= 1028 and _lib.MIN_VERSION >= 1028
    assert _lib.load(True).pm_version() >= _lib.MIN_VERSION


# ------------------------------------------------------------------------------------------------------- the plan table
@pytest.mark.parametrize("H,vpl", [(1, 1), (64, 1), (65, 2), (128, 2), (129, 4), (256, 4), (257, 8), (512, 8), (513, 16), (1024, 16)])
def test_select_vpl(H, vpl):
    for N, grid in ((1, 1), (5, 2), (9000, 2048)):
        rc, out = plan(R.SELECT, H, 0, min(H, 5), 0, 0, 0, N)
        assert rc == PM_OK and out[:R.O_GRID + 1] == (R.WAVE, vpl, 0, 0, 0, 0, 0, 0, grid), (H, N, out)
        assert out[R.O_GRID + 1:] == (0,) * 5


@pytest.mark.parametrize("which", [R.ESTEP, R.MSTEP_ROWS])
def test_wave_lds(which):
    """LDS bytes of the two generic kernels as their layouts spell them; grid = ceil(N / 4) up to 2048."""
    for H, Hp, gamma in ((5, 3, 2), (12, 5, 3), (70, 6, 3), (1024, 16, 2)):
        S = R.n_states(Hp, gamma)
        ptr, lst = R.pair_lists(R.state_matrix(Hp, gamma))
        want = 8 * (H + 4 * (16 + 256)) + 2 * S if which == R.ESTEP else \
            8 * (2 * H + 4 * (H + S) + 12) + 4 * (Hp * Hp + 1) + 2 * (S + len(lst))
        for N in (1, 4, 5):
            rc, out = plan(which, H, 8, Hp, S, gamma, 0, N)
            assert rc == PM_OK and (out[R.O_FAMILY], out[R.O_LDS], out[R.O_GRID]) == (R.WAVE, want, -(-N // 4)), (H, out)
    assert plan(which, 70, 8, 6, 0, 1, 0, 5)[0] == PM_OK                      # S = 0


def _rows16_layout_bytes(H, Hp, S, rowbuf):
    """make_layout of bsc_rows16_body.h, restated from its LDS map."""
    HT = (H + 15) // 16 * 16
    p_len = max(1 + 16 + Hp * Hp + S, 17 * 16)
    area = p_len + 16 + (HT if rowbuf else 0)
    off_tab = 4 * HT * 8 + 16 * area * 8
    off_st = (off_tab + 4 * S + 15) // 16 * 16
    return (off_st + 16 * S + 2 * Hp * Hp + 15) // 16 * 16


def _mstep16_bytes(H, Hp, S, lists):
    b = 8 * (2 * H + 16 * Hp * Hp + 12) + 2 * S
    return (b + 7) // 8 * 8 + 8 * 16 * H if lists else b


@pytest.mark.parametrize("H,vpl", [(1, 1), (16, 1), (17, 2), (32, 2), (33, 4), (64, 4), (65, 8), (128, 8), (129, 16), (256, 16), (257, 32),
                                   (512, 32)])
def test_rows16_vpl(H, vpl):
    Hp, gamma = min(H, 5), min(H, 3)
    S = R.n_states(Hp, gamma)
    for mode in (1, 2, 3, 1 | 4, 1 | 8, 1 | 16):
        rc, out = plan(R.SELECT_ESTEP, H, 0, Hp, S, gamma, mode, 65)
        assert rc == PM_OK and out[:R.O_GRID + 1] == (R.LANES16, vpl, 0, 0, 0, 0, (mode >> 1) & 1, _rows16_layout_bytes(H, Hp, S, 0), 5), out
    for lists in (0, R.F_LISTS):
        rc, out = plan(R.MSTEP_ROWS16, H, 8, Hp, S, gamma, lists, 17)
        if lists and H > 256:
            assert rc == PM_ERANGE
        else:
            assert rc == PM_OK and out[:R.O_GRID + 1] == (R.LANES16, vpl, 0, 0, 0, 0, 1 if lists else 0,
                                                           _mstep16_bytes(H, Hp, S, lists), 2), out
    assert plan(R.SELECT_ESTEP, H, 0, Hp, S, gamma, 3, 16 * 2048 + 1)[1][R.O_GRID] == 2048          # the persistent grid's cap


@pytest.mark.parametrize("H,nj,full", [(16, 8, 0), (127, 8, 0), (128, 8, 1), (129, 16, 0), (255, 16, 0), (256, 16, 1)])
def test_fused_nj(H, nj, full):
    Hp, gamma = 5, 3
    S = R.n_states(Hp, gamma)
    for stats in (0, R.F_STATS):
        for D in (8, 24, 32, 40):
            rc, out = plan(R.FUSED, H, D, Hp, S, gamma, 3 | stats, 129)
            ring = 8 * 4 * (64 + 16 * nj) * 8
            assert rc == PM_OK and out[:R.O_GRID + 1] == (R.FAM_FUSED, 0, nj, 0, 0, full, 1 if stats else 0,
                                                           max(ring, _rows16_layout_bytes(H, Hp, S, 1)), 3), (H, D, out)
    assert plan(R.FUSED, 257, 8, Hp, S, gamma, 3, 1)[0] == PM_ERANGE


@pytest.mark.parametrize("hp", [5, 6, 7, 8])
@pytest.mark.parametrize("gamma", [3, 4])
def test_fused8_instantiations(hp, gamma):
    S = R.n_states(hp, gamma)
    for H, full in ((129, 0), (200, 0), (255, 0), (256, 1)):
        for flags, ms in ((1, 0), (2, 0), (3, 0), (3 | R.F_STATS, 1), (3 | R.F_STATS | R.F_LISTS, 1)):
            rc, out = plan(R.FUSED8, H, 8, hp, S, gamma, flags, 33)
            assert rc == PM_OK and out == (R.FAM_FUSED8, 0, 8, hp, gamma, full, ms, 157184, 3, 0, 0, 33, 3, 147456), (H, flags, out)
    for H in (128, 257):
        assert plan(R.FUSED8, H, 8, hp, S, gamma, 3, 33)[0] == PM_ERANGE


# ------------------------------------------------------------------------------------------------------ PM_ERANGE edges
def test_erange_edges():
    S53 = R.n_states(5, 3)
    for which in (R.SELECT, R.ESTEP, R.MSTEP_ROWS):
        assert plan(which, 4, 8, 5, 0, 1, 0, 1)[0] == PM_ERANGE                      # Hprime > H
        assert plan(which, 1025, 8, 5, 0, 1, 0, 1)[0] == PM_ERANGE                   # H > PM_MAX_H
        assert plan(which, 40, 8, 17, 0, 1, 0, 1)[0] == PM_ERANGE                    # Hprime > PM_MAX_HPRIME
    for which in (R.ESTEP, R.MSTEP_ROWS):
        assert plan(which, 40, 8, 5, 65536, 3, 0, 1)[0] == PM_ERANGE
    assert plan(R.ESTEP, 40, 8, 5, 65535, 3, 0, 1)[0] == PM_OK                       # 9024 + 131070 bytes
    assert plan(R.MSTEP_ROWS, 1024, 8, 16, 3000, 16, 0, 1)[0] == PM_ERANGE           # the LDS layout above 160 KB
    for which, fl in ((R.SELECT_ESTEP, 3), (R.MSTEP_ROWS16, 0)):
        assert plan(which, 4, 8, 5, 0, 1, fl, 1)[0] == PM_ERANGE                     # Hprime > H
        assert plan(which, 513, 8, 5, S53, 3, fl, 1)[0] == PM_ERANGE
        assert plan(which, 40, 8, 17, 0, 1, fl, 1)[0] == PM_ERANGE
        assert plan(which, 40, 8, 5, 4097, 3, fl, 1)[0] == PM_ERANGE
        assert plan(which, 512, 8, 16, 4096, 3, fl, 1)[0] == PM_ERANGE               # the selection layout above 156 KB
    assert plan(R.MSTEP_ROWS16, 257, 8, 5, S53, 3, R.F_LISTS, 1)[0] == PM_ERANGE     # lists: H > 256
    # (the list layout itself, at most 71 KB at H = 256, H' = 16, never decides: it fits wherever the selection layout does)
    assert _lib().pm_bsc_rows16_supported(256, 16, 680) == 1 and _lib().pm_bsc_rows16_nz_supported(256, 16, 680) == 1
    assert _lib().pm_bsc_rows16_supported(257, 16, 680) == 1 and _lib().pm_bsc_rows16_nz_supported(257, 16, 680) == 0
    for D in (4, 7, 9, 12):
        assert plan(R.FUSED, 64, D, 5, S53, 3, 3, 1)[0] == PM_ERANGE                 # D not a multiple of 8
        assert plan(R.FUSED8, 200, D, 5, S53, 3, 3, 1)[0] == PM_ERANGE
    assert plan(R.FUSED, 64, 8, 5, S53, 3, 3 | 4, 1)[0] == PM_ERANGE                 # BSC's own ranking only
    assert plan(R.FUSED, 64, 8, 9, R.n_states(9, 3), 3, 3 | R.F_STATS, 1)[0] == PM_ERANGE      # stats with Hprime > 8
    assert plan(R.FUSED, 64, 8, 9, R.n_states(9, 3), 3, 3, 1)[0] == PM_OK
    assert plan(R.FUSED, 256, 8, 16, 2516, 3, 3, 1)[0] == PM_ERANGE                  # the epilogue's layout above 80 KB
    for hp in (4, 9):
        assert plan(R.FUSED8, 200, 8, hp, R.n_states(hp, 3), 3, 3, 1)[0] == PM_ERANGE
    for H in (1, 128, 257):
        assert plan(R.FUSED8, H, 8, 5, S53, 3, 3, 1)[0] == PM_ERANGE
    assert plan(R.FUSED8, 200, 8, 5, S53 - 1, 3, 3, 1)[0] == PM_ERANGE               # not a complete state set
    assert plan(R.FUSED8, 200, 8, 5, S53, 4, 3, 1)[0] == PM_ERANGE                   # ... of this gamma
    assert plan(R.FUSED8, 200, 8, 5, R.n_states(5, 2), 2, 3, 1)[0] == PM_ERANGE
    assert plan(R.FUSED8, 200, 8, 6, R.n_states(6, 5), 5, 3, 1)[0] == PM_ERANGE
    assert plan(R.FUSED8, 200, 8, 5, S53, 3, 3 | 8, 1)[0] == PM_ERANGE
    # a shard whose row counts do not fit out[]
    assert plan(R.FUSED8, 200, 8, 5, S53, 3, 3, 2 ** 31 - 1)[0] == PM_OK and plan(R.FUSED8, 200, 8, 5, S53, 3, 3, 2 ** 31 + 5)[0] == PM_ERANGE


def test_einval():
    S53 = R.n_states(5, 3)
    out = (ctypes.c_int32 * R.PLAN_LEN)()
    assert _lib().pm_bsc_plan(R.FUSED8, 200, 8, 5, S53, 3, 3, 1, 256, None) == PM_EINVAL
    for which in (-1, 7):
        assert _lib().pm_bsc_plan(which, 200, 8, 5, S53, 3, 3, 1, 256, out) == PM_EINVAL
    for which in range(7):
        fl = 3 if which in (R.SELECT_ESTEP, R.FUSED, R.FUSED8) else 0
        H = 200 if which == R.FUSED8 else 64
        assert plan(which, H, 8, 5, S53, 3, fl, 1)[0] == PM_OK, which
        assert plan(which, 0, 8, 5, S53, 3, fl, 1)[0] == PM_EINVAL and plan(which, H, 8, 0, S53, 3, fl, 1)[0] == PM_EINVAL
        assert plan(which, H, 8, 5, S53, 3, fl, 0)[0] == PM_EINVAL and plan(which, H, 8, 5, -1, 3, fl, 1)[0] == PM_EINVAL
        assert plan(which, H, 8, 5, S53, 3, fl | 128, 1)[0] == PM_EINVAL                # an unknown flag
    assert plan(R.SELECT, 64, 8, 5, 0, 0, 1, 1)[0] == PM_EINVAL                          # a flag the entry does not have
    assert plan(R.MSTEP_ROWS16, 64, 8, 5, S53, 3, R.F_STATS, 1)[0] == PM_EINVAL
    for which, H in ((R.SELECT_ESTEP, 64), (R.FUSED, 64), (R.FUSED8, 200)):
        assert plan(which, H, 8, 5, S53, 3, 0, 1)[0] == PM_EINVAL                        # neither mode bit
        assert plan(which, H, 8, 5, S53, 0, 3, 1)[0] == PM_EINVAL and plan(which, H, 8, 5, S53, 6, 3, 1)[0] == PM_EINVAL
    for which, H in ((R.FUSED, 64), (R.FUSED8, 200)):
        assert plan(which, H, 0, 5, S53, 3, 3, 1)[0] == PM_EINVAL
        assert plan(which, H, 8, 5, S53, 3, 1 | R.F_STATS, 1)[0] == PM_EINVAL            # statistics without the E-step
    assert plan(R.FUSED8, 200, 8, 5, S53, 3, 3 | R.F_LISTS, 1)[0] == PM_EINVAL           # lists without statistics


# ------------------------------------------------------------------------------------------------------- the predicates
def test_plan_agrees_with_the_predicates():
    lib = _lib()
    for H in (1, 5, 16, 17, 100, 128, 129, 200, 256, 257, 512, 513):
        for Hp in (1, 4, 5, 8, 9, 16, 17):
            for gamma in (1, 2, 3, 4):
                if gamma > Hp:
                    continue
                S = R.n_states(Hp, gamma) if Hp <= 16 else 0
                ok = lambda rc: 1 if rc == PM_OK else 0
                assert ok(plan(R.SELECT_ESTEP, H, 0, Hp, S, gamma, 3, 1)[0]) == lib.pm_bsc_rows16_supported(H, Hp, S)
                assert ok(plan(R.MSTEP_ROWS16, H, 8, Hp, S, gamma, 0, 1)[0]) == lib.pm_bsc_rows16_supported(H, Hp, S)
                assert ok(plan(R.MSTEP_ROWS16, H, 8, Hp, S, gamma, R.F_LISTS, 1)[0]) == lib.pm_bsc_rows16_nz_supported(H, Hp, S)
                for D in (4, 8, 12, 64):
                    assert ok(plan(R.FUSED, H, D, Hp, S, gamma, 3, 1)[0]) == lib.pm_bsc_fused_supported(H, D, Hp, S), (H, Hp, gamma, D)
                    whole = lib.pm_bsc_fused8_supported(H, D, Hp, S) and lib.pm_bsc_fused8_whole_shard(H, Hp, gamma, S)
                    assert ok(plan(R.FUSED8, H, D, Hp, S, gamma, 3, 1)[0]) == (1 if whole else 0), (H, Hp, gamma, D)
                    # no device here: the occupancy query answers <= 0, and 0 exactly where the shape is unsupported
                    occ = lib.pm_bsc_fused_occupancy(H, D, Hp, S)
                    assert (occ == 0) == (not lib.pm_bsc_fused_supported(H, D, Hp, S)), (H, Hp, gamma, D, occ)
    # either complete state set passes pm_bsc_fused8_supported; the launch needs the one of its gamma
    assert lib.pm_bsc_fused8_supported(200, 8, 6, R.n_states(6, 4)) == 1 and lib.pm_bsc_fused8_whole_shard(200, 6, 3, R.n_states(6, 4)) == 0


# ------------------------------------------------------------------------------------------------------ the fused8 split
@pytest.mark.parametrize("cus", [256, 104])
def test_fused8_split(cus):
    """The rule in the launcher's comment: whole rounds of cus 128 rows go to the main launch; a ragged round goes with them
    when it fills at least 70 % of a round or exceeds two rounds of 16-row TAIL workgroups; else to the TAIL launch."""
    S, rnd, two = R.n_states(8, 4), cus * 128, 2 * cus * 16
    seventy = -(-7 * rnd // 10)

    def split(N):
        rc, out = plan(R.FUSED8, 256, 64, 8, S, 4, 3, N, cus)
        assert rc == PM_OK and out[R.O_MAIN_ROWS] + out[R.O_TAIL_ROWS] == N
        assert out[R.O_MAIN_GRID] == -(-out[R.O_MAIN_ROWS] // 128) and out[R.O_TAIL_GRID] == -(-out[R.O_TAIL_ROWS] // 16)
        assert out[R.O_GRID] == out[R.O_MAIN_GRID] + out[R.O_TAIL_GRID]
        return out[R.O_MAIN_ROWS]
    assert split(1) == 0 and split(two) == 0                       # all TAIL
    assert split(two + 1) == two + 1                               # all main
    assert split(rnd) == rnd
    for r, main in ((1, rnd), (two, rnd), (two + 1, rnd + two + 1), (seventy - 1, rnd + seventy - 1), (seventy, rnd + seventy)):
        assert split(rnd + r) == main, (cus, r)
    assert two < seventy                                           # (so the 70 % rule never decides alone: documented, not reachable)
    assert split(3 * rnd + 17) == 3 * rnd
    if cus == 256:
        assert _lib().pm_bsc_fused8_main_rows(200000, 64) == 6 * rnd       # config 2 (no device: 256 compute units assumed)
        assert _lib().pm_bsc_fused8_main_rows(8193, 64) == 8193 and _lib().pm_bsc_fused8_main_rows(8192, 64) == 0


# ------------------------------------------------------------------------------------------------------- the case table
CASE_NAMES = [n for n, sp in R.CASES.items() if sp["entry"] == "fused8"]
OTHER_NAMES = [n for n, sp in R.CASES.items() if sp["entry"] != "fused8"]


@pytest.mark.parametrize("cus", [256, 304])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_case_cell_and_exactness(name, cus):
    """The plan sends every row of the case to the launch it is named after, in its instantiation; the operands are exact:
    integers, |W_h| a power of two, ranking keys of fewer than 32 significant bits, energies integers below 2^30, ecoef e + prior
    exact in float64; a tie at the H' boundary; hot: all weights of a row within a factor e."""
    spec = R.CASES[name]
    hp, g, full, ms, tail = spec["cell"]
    for hot in (True, False):
        c = R.make_case(name, hot, cus=cus)
        rc, out = plan(R.FUSED8, c["H"], c["D"], c["Hp"], c["S"], c["gamma"], 3 | (R.F_STATS if c["stats"] else 0), c["N"], cus)
        assert rc == PM_OK and out[:R.O_MSTATS + 1] == (R.FAM_FUSED8, 0, 8, hp, g, full, ms), (name, out)
        N = c["N"]
        assert out[R.O_MAIN_ROWS:R.O_TAIL_ROWS + 1] == {1: (0, 0, N), 0: (N, -(-N // 128), 0), 2: (cus * 128, cus, 17)}[tail], (name, out)
        for k in ("Y", "Wt", "A", "G", "yn2"):
            assert (c[k] == np.rint(c[k])).all() and np.abs(c[k]).max() < 2 ** 20, (name, k)
        assert np.array_equal(c["A"], c["Y"] @ c["Wt"].T) and np.array_equal(c["G"], c["Wt"] @ c["Wt"].T)
        assert c["ecoef"] in (-2.0, -2.0 ** -20) and c["prior_scale"] in (1.0, 0.5) and c["pil_bar"] * 16 == np.rint(c["pil_bar"] * 16)
        ref = R.case_reference(c)
        assert ref["exact"] and ref["boundary_ties"] > 0, name
        prod = c["ecoef"] * ref["E"].astype(np.float64)
        assert (prod.astype(LD) == LD(c["ecoef"]) * ref["E"]).all(), name
        given = R.case_reference(c, cand=c["cand_in"])
        assert given["exact"] and all(len(set(r)) == c["Hp"] for r in c["cand_in"][:c["rows"]].tolist())
        if hot:
            for rf in (ref, given):
                w = rf["F"] - rf["lse"][:, None]
                assert float((w.max(axis=1) - w.min(axis=1)).max()) < 1.0, name
        else:
            cnt = R.row_stats(ref["F"], ref["lse"], np.ones(c["rows"], dtype=bool), ref["E"], ref["cand"], c["SM"], c["H"],
                              c["ecoef"], drop=R.dropped_onepass(ref["F64"]))["nz_cnt"]
            assert R.dropped_onepass(ref["F64"]).any(), (name, "no term below the cut-off")
            if name in R.LIST_CASES:
                assert (cnt <= R.NZ_MAX).any() and (name == "tail_hp6_g4_part_ms" or (cnt > R.NZ_MAX).any()), (name, cnt)
                want = {"tail_hp6_g4_part_ms": R.NZ_MAX, "tail_hp6_g3_part_ms": R.NZ_MAX + 1, "main_hp8_g4_full_ms": R.NZ_MAX + 1}
                assert name not in want or (cnt == want[name]).any(), (name, cnt)


def _other_cells(sp, c):
    """The plan cells a case of the other launchers runs in: (which, flags) -> the fields that tell the cells apart."""
    H, D, Hp, S, g = c["H"], c["D"], c["Hp"], c["S"], c["gamma"]
    e = sp["entry"]
    calls = {"select": [(R.SELECT, 0)], "wave": [(R.ESTEP, 0), (R.MSTEP_ROWS, 0)],
             "select_estep": [(R.SELECT_ESTEP, m) for m in (1, 2, 3, 1 | 4, 1 | 8, 1 | 16)],
             "rows16": [(R.MSTEP_ROWS16, 0), (R.MSTEP_ROWS16, R.F_LISTS)],
             "fused": [(R.FUSED, 3 | (R.F_STATS if sp["stats"] else 0))]}[e]
    cells = set()
    for which, fl in calls:
        rc, out = plan(which, H, D, Hp, S, g, fl, c["N"])
        if rc == PM_OK:
            cells.add((which, out[R.O_FAMILY], out[R.O_VPL], out[R.O_NJ], out[R.O_FULL], out[R.O_MSTATS]))
        else:
            assert rc == PM_ERANGE and which == R.MSTEP_ROWS16 and fl and H > 256, (sp, which, fl, rc)
    return cells


@pytest.mark.parametrize("name", OTHER_NAMES)
def test_other_case_cell_and_exactness(name):
    """The cases of the other launchers: the plan reports the cell the case table names; exact operands, a tie at the H'
    boundary, hot: all weights of a row within a factor e; cold: terms below the cut-offs (where the kernel has one)."""
    sp = R.CASES[name]
    for hot in (True, False):
        c = R.make_case(name, hot)
        for cell in _other_cells(sp, c):
            fam_first = (cell[1],) + ((cell[2],) if cell[1] in (R.WAVE, R.LANES16) and len(sp["cell"]) > 1 else ())
            if sp["entry"] == "fused":
                assert (cell[1], cell[3], cell[4], cell[5]) == sp["cell"], (name, cell)
            else:
                assert fam_first == sp["cell"], (name, cell)
        for k in ("Y", "Wt", "A", "G", "yn2"):
            assert (c[k] == np.rint(c[k])).all() and np.abs(c[k]).max() < 2 ** 20, (name, k)
        assert np.array_equal(c["A"], c["Y"] @ c["Wt"].T) and np.array_equal(c["G"], c["Wt"] @ c["Wt"].T)
        ref = R.case_reference(c)
        assert ref["exact"] and ref["boundary_ties"] > 0, name
        prod = c["ecoef"] * ref["E"].astype(np.float64)
        assert (prod.astype(LD) == LD(c["ecoef"]) * ref["E"]).all(), name
        for mode in (1 | 4, 1 | 8, 1 | 16):                       # the other ranking keys are integers
            X = c["G"].diagonal()[None, :] - 2 * c["A"] if mode & 16 else c["A"]
            assert (X == np.rint(X)).all() and np.abs(X).max() < 2 ** 20
        if hot:
            w = ref["F"] - ref["lse"][:, None]
            assert float((w.max(axis=1) - w.min(axis=1)).max()) < 1.0, name
            if name in ("r16_h16", "r16_h17"):
                assert c["H"] == R.NZ_MAX + (name == "r16_h17")     # hot: every latent of every row is a non-zero
        elif sp["entry"] in ("rows16", "fused", "select_estep"):
            l64 = ref["lse"].astype(np.float64)
            assert R.dropped(ref["F64"], l64, R.QCUT).any() and R.dropped_onepass(ref["F64"]).any(), name


def test_every_cell_of_the_other_launchers_has_a_case():
    """Every (entry, family, VPL, NJ, FULL, MSTATS) cell pm_bsc_plan can report for pm_bsc_select_f64, the generic kernels,
    pm_bsc_select_estep_f64 (every mode the tests use), pm_bsc_mstep_rows16_f64 / _nz_f64 and pm_bsc_estep_fused_f64 -- swept
    over every H the entry admits -- is the cell of at least one case."""
    have = set()
    for name in OTHER_NAMES:
        have |= _other_cells(R.CASES[name], R.make_case(name, True))
    need = set()
    S53 = R.n_states(5, 3)
    for H in range(5, 1025):
        sweeps = [(R.SELECT, 0), (R.ESTEP, 0), (R.MSTEP_ROWS, 0)] + [(R.SELECT_ESTEP, m) for m in (1, 2, 3, 5, 9, 17)] + \
            [(R.MSTEP_ROWS16, 0), (R.MSTEP_ROWS16, R.F_LISTS), (R.FUSED, 3), (R.FUSED, 3 | R.F_STATS)]
        for which, fl in sweeps:
            rc, out = plan(which, H, 8, 5, S53, 3, fl, 17)
            if rc == PM_OK:
                need.add((which, out[R.O_FAMILY], out[R.O_VPL], out[R.O_NJ], out[R.O_FULL], out[R.O_MSTATS]))
    assert need <= have, sorted(need - have)
    entries = {sp["entry"] for sp in R.CASES.values()}
    assert entries == {"fused8", "select", "wave", "select_estep", "rows16", "fused"}
    fused = [sp for sp in R.CASES.values() if sp["entry"] == "fused"]
    assert {sp["N"] for sp in fused} == {1, 63, 64, 65, 129} and {sp["D"] for sp in fused} == {8, R.RING_K - 8, R.RING_K, R.RING_K + 8}
    se = [sp for sp in R.CASES.values() if sp["entry"] == "select_estep"]
    assert {sp["N"] for sp in se} == {1, 15, 16, 17, 65} and {sp["gamma"] for sp in se} == {1, 3, 5}
    wave = [sp for sp in R.CASES.values() if sp["entry"] == "wave"]
    assert {(sp["H"], sp["Hp"], sp["gamma"]) for sp in wave} >= {(5, 3, 2), (12, 5, 3), (70, 6, 3)} and {sp["N"] for sp in wave} == {1, 4, 5}
    assert any(sp["gamma"] == 1 for sp in wave) and any(sp["mu"] for sp in wave)


def test_every_cell_has_a_case():
    """The 64 instantiations <HP, GAMMA, FULL, MSTATS, TAIL> of bsc_estep_fused8s_kernel, the call that makes both launches,
    mu on either launch; and the shapes the edges sit at: every H, N and D of the list, on the launch it belongs to."""
    cells = {s["cell"] for s in R.CASES.values() if s["entry"] == "fused8"}
    for hp in (5, 6, 7, 8):
        for g in (3, 4):
            for full in (0, 1):
                for ms in (0, 1):
                    for tail in (0, 1):
                        assert (hp, g, full, ms, tail) in cells, (hp, g, full, ms, tail)
    f8 = [s for s in R.CASES.values() if s["entry"] == "fused8"]
    assert any(s["cell"][4] == 2 for s in f8)
    tails = [s for s in f8 if s["cell"][4] == 1]
    mains = [s for s in f8 if s["cell"][4] == 0]
    assert {s["H"] for s in tails} == {129, 200, 256} and {s["N"] for s in tails} == {1, 15, 16, 17, 33}
    assert {s["D"] for s in tails} == {8, 16, 32, 40}
    assert {s["H"] for s in mains} == {129, 255, 256} and {s["N"] for s in mains} == {"main"}
    assert {s["D"] for s in mains} == {8, R.RING_K, R.RING_K + 8}
    assert any(s["mu"] for s in tails) and any(s["mu"] and s["H"] == 256 and s["Hp"] == 8 and s["gamma"] == 4 for s in mains)


# ----------------------------------------------------------------------------------------------------- the reference
def test_reference_agrees_with_the_oracle():
    """Selection, log-joints and statistics of bsc_kernels_reference against oracle/bsc_oracle.py on a small random model
    (1e-12: the oracle works in float64)."""
    from oracle import bsc_oracle as O
    rng = np.random.RandomState(7)
    D, H, Hp, gamma, N = 9, 14, 5, 3, 23
    W = rng.normal(size=(D, H))
    Y = rng.normal(size=(N, D)) + 0.5
    mu = rng.normal(size=D) * 0.1
    pies, sigma, T = 0.15, 1.3, 1.2
    _, S, SM, state_abs = O.generate_state_matrix(Hp, gamma)
    assert np.array_equal(SM, R.state_matrix(Hp, gamma)) and S == R.n_states(Hp, gamma)
    Wt = W.T.copy()
    A, g = Y @ Wt.T, (Wt * Wt).sum(axis=1)
    cand = R.select(A, g, Hp, yn2=(Y * Y).sum(axis=1))
    assert np.array_equal(cand, O.select_hprimes_loop(W, Y, Hp)) and np.array_equal(cand, R.select(A, g, Hp))
    for anneal_prior in (False, True):
        anneal = O.Anneal(T=T, anneal_prior=anneal_prior)
        want = O.e_step_loop(anneal, W, pies, sigma, mu, Y, cand, SM, state_abs)
        ecoef = -(1.0 / T) / (2 * sigma * sigma)
        E = R.energies(Y, Wt, mu, cand, R.state_matrix(Hp, gamma))
        F = R.log_joints(E, R.state_sizes(H, R.state_matrix(Hp, gamma)), np.log(pies / (1 - pies)), ecoef,
                         1.0 / T if anneal_prior else 1.0)
        np.testing.assert_allclose(F.astype(np.float64), want, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(E.astype(np.float64), O.energies_vec(W, mu, Y, cand, SM), rtol=1e-12, atol=1e-12)
        l = R.lse(F)
        np.testing.assert_allclose(l.astype(np.float64), np.log(np.exp(want).sum(axis=1)), rtol=1e-12)
        keep = np.arange(N) % 3 != 1
        st = R.row_stats(F, l, keep, E, cand, R.state_matrix(Hp, gamma), H, ecoef)
        o = O.m_step_stats_loop(W, mu, Y[keep], cand[keep], want[keep], SM)
        mus = (st["q1"] + st["m1"]).astype(np.float64)
        np.testing.assert_allclose(mus, o["mus"], rtol=1e-12)
        np.testing.assert_allclose(float(st["sig"]), o["sigma"], rtol=1e-12)
        np.testing.assert_allclose((st["expect"][keep].T @ (Y[keep] - mu)).astype(np.float64), o["Wp"], rtol=1e-11, atol=1e-12)
        assert not st["expect"][~keep].any() and float(st["cnt"]) == keep.sum()
        up = st["upper"].astype(np.float64)
        np.testing.assert_allclose(up + up.T + np.diag(mus), o["Wq"], rtol=1e-12, atol=1e-14)
        # the three packed conventions assemble to the same matrix: upper + upper^T - diag(upper) + diag(qdiag)
        sec = R.stats_sections(H, D)
        for conv in ("rows", "fused", "fused8"):
            p = R.pack_stats(st, H, D, conv).astype(np.float64)
            Wq, qd, m = p[sec["Wq"]].reshape(H, H), p[sec["qdiag"]], p[sec["mus"]]
            if conv == "fused":
                qd = m - np.diag(Wq)
            full = Wq + Wq.T - np.diag(np.diag(Wq)) + np.diag(qd)
            np.testing.assert_allclose(full, o["Wq"], rtol=1e-12, atol=1e-14, err_msg=conv)
        # the records hold the pair blocks and ecoef sum q e of every row, kept or not
        n = 1
        q = np.exp(F[n] - l[n])
        assert abs(float(st["records"][n, 36] - LD(ecoef) * (q * E[n]).sum())) < 1e-15
        B = (SM.astype(LD) * q[1 + H:, None]).T @ SM.astype(LD)
        assert abs(float(st["records"][n, R.pair_entry(1, 3)] - B[1, 3])) < 1e-18 and st["records"][n, R.pair_entry(2, 2)] == 0
    # the tie rule: of equal similarities the larger index ranks higher; smallest-first the smaller index first
    X = np.array([[1.0, 3.0, 3.0, 0.0, 3.0, 1.0]])
    assert R.rank_best_last(X, 2).tolist() == [[2, 4]] and R.rank_best_last(X, 4).tolist() == [[5, 1, 2, 4]]
    assert R.rank_smallest_first(X, 2).tolist() == [[3, 0]]
    # lists
    idx, cnt = R.lists_of(np.array([[0, 1.0, 0, 2.0], [0, 0, 0, 0]]))
    assert idx[0, :3].tolist() == [1, 3, R.NZ_PAD] and cnt.tolist() == [2, 0] and (idx[1] == R.NZ_PAD).all()
