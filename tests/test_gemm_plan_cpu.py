"""pm_gemm_nt_plan / pm_gemm_tn_plan: the dispatch decisions of pm_gemm_nt_f64 and pm_gemm_tn_acc_gated_f64 as host-only
queries (the launchers switch on the same functions).  No device is needed: without one the libraries assume 256 CUs, i.e.
512 resident workgroup slots, and every expected mask below is worked out by hand for the slot count the library reports.

The shape helpers are shared with tests/test_dense_kernels_gpu.py, which asserts the same masks on the device before it
checks what the kernels computed."""
import ctypes

import pytest

# PM_NT_PLAN_* / PM_TN_PLAN_* of include/prosper_hip.h
NT_MAIN, NT_REST, NT_REST_SPLIT, NT_FUSED, NT_REST64 = 0x001, 0x002, 0x004, 0x008, 0x010
NT_MT1, NT_MT2, NT_MT4, NT_ALIGNED, NT_WHOLE = 0x020, 0x040, 0x080, 0x100, 0x200
TN_DMA, TN_REG, TN_ALIGNED, TN_REMAP, TN_TAIL = 0x01, 0x02, 0x04, 0x08, 0x10
PM_EINVAL, PM_ERANGE = -1, -2
INT32_MAX = 2 ** 31 - 1


def nt_plan(M, N, K, aligned, det=False):
    """(mask, [slots, main_panels, nsplit]) of pm_gemm_nt_plan."""
    from prosper_amd import _lib
    out = (ctypes.c_int32 * 3)(-7, -7, -7)
    mask = _lib.load(det).pm_gemm_nt_plan(M, N, K, int(aligned), out)
    return mask, list(out)


def tn_plan(M, N, K, aligned, det=False):
    """(mask, [slots, nsplit, rows of K per split]) of pm_gemm_tn_plan."""
    from prosper_amd import _lib
    out = (ctypes.c_int32 * 3)(-7, -7, -7)
    mask = _lib.load(det).pm_gemm_tn_plan(M, N, K, int(aligned), out)
    return mask, list(out)


def slots_of(det=False):
    return nt_plan(1, 1, 1, 0, det)[1][0]


def nt_path_cases(slots):
    """name -> (M, N, K, aligned, mask of the default build, mask of the deterministic build): the smallest shapes that reach
    every path of pm_gemm_nt_f64 on a device with `slots` resident workgroups (a multiple of 32, at least 64).  At 512
    slots: main (16384, 512, 8), fused (16517, 512, 128), 64-row (10245, 1024, 8), MT = 2 (4128, 500, .), MT = 4
    (8200, 512, .).

    Why each shape takes its path (tn = ceil(N / 128) column tiles, a round = slots tiles):
      main      slots / 4 panels of 4 tiles: exactly one round, nothing left
      fused     + 133 rows = 2 panels = 8 tiles behind the round; K = 128 is 16 K-steps: 2 slices of 8
      rest64    slots / 8 panels of 8 tiles (one round) + (slots / 32 + 1) panels = slots / 4 + 8 tiles: between a quarter and
                70 % of a round, and K = 8 is one K-step, which cannot be split; the deterministic build runs all of it as
                one launch of 128-row tiles, as it does for `fused`
      split     4 tiles, 128 K-steps: min(slots / 4, 128 / 8) = 16 slices; the deterministic build never splits
      rest      2 tiles, 6 K-steps: fewer than the 8 a slice needs
      mt1 ...   K % 8 != 0 goes to the register-staged kernels: 32-row tiles while they fit the slots (5 x 2, 11 x 1), 64-row
                tiles when 128-row tiles fill at most half of them (slots / 16 + 1 panels x 4) but 32-row tiles would not fit
                (slots + 4), 128-row tiles otherwise (2 x (slots / 8 + 1) x 4 > slots) and for M <= 32
      *_odd_base   an 8-byte-aligned base with K % 8 == 0 must NOT take the LDS-DMA kernel (16-byte loads)"""
    assert slots % 32 == 0 and slots >= 64
    A = NT_ALIGNED
    m_main = 128 * (slots // 4)
    m_mt2 = 32 * (slots // 4) + 32
    m_mt4 = 128 * (slots // 8) + 8
    return {
        "main": (m_main, 512, 8, 1, NT_MAIN | A, NT_MAIN | A),
        "fused": (m_main + 128 + 5, 512, 128, 1, NT_FUSED | A, NT_WHOLE | A),
        "rest64": (128 * (slots // 8) + (slots // 32) * 128 + 5, 1024, 8, 1, NT_MAIN | NT_REST64 | A, NT_WHOLE | A),
        "split": (200, 256, 1024, 1, NT_REST_SPLIT | A, NT_REST | A),
        "rest": (64, 100, 48, 1, NT_REST | A, NT_REST | A),
        "mt1_al": (130, 129, 18, 1, NT_MT1 | A, NT_MT1 | A),
        "mt1_un": (333, 10, 25, 1, NT_MT1, NT_MT1),
        "mt2_un": (m_mt2, 500, 9, 1, NT_MT2, NT_MT2),
        "mt2_al": (m_mt2, 500, 18, 1, NT_MT2 | A, NT_MT2 | A),
        "mt4_un": (m_mt4, 512, 9, 1, NT_MT4, NT_MT4),
        "mt4_al": (m_mt4, 512, 18, 1, NT_MT4 | A, NT_MT4 | A),
        "mt4_one": (1, 1, 1, 1, NT_MT4, NT_MT4),
        "mt4_odd_base": (32, 16, 8, 0, NT_MT4, NT_MT4),
        "mt1_odd_base": (200, 256, 1024, 0, NT_MT1, NT_MT1),
    }


def tn_path_cases():
    """name -> (M, N, K, aligned, mask, nsplit) of pm_gemm_tn_acc_gated_f64, the same in both builds and for any slot count
    from 64 up: at most ceil(K / 128) splits (8 K-steps of 16 rows each at least), the LDS-DMA kernel for whole 128 x 128
    tiles of aligned operands with K >= 64, the XCD remap when the splits are a multiple of 8."""
    return {
        "dma": (128, 128, 64, 1, TN_DMA | TN_ALIGNED, 1),
        "dma_tail": (128, 128, 71, 1, TN_DMA | TN_ALIGNED | TN_TAIL, 1),
        "dma_remap": (128, 256, 1024, 1, TN_DMA | TN_ALIGNED | TN_REMAP, 8),
        "reg_al_edge_m": (130, 128, 64, 1, TN_REG | TN_ALIGNED, 1),
        "reg_al_short_k": (128, 128, 63, 1, TN_REG | TN_ALIGNED, 1),
        "reg_un": (33, 7, 5, 1, TN_REG, 1),
        "reg_odd_base": (128, 128, 64, 0, TN_REG, 1),
        "reg_remap": (130, 128, 1024, 1, TN_REG | TN_ALIGNED | TN_REMAP, 8),
    }


DET = [False, True]


@pytest.mark.parametrize("det", DET)
def test_plans_validate_like_the_launchers(det):
    """PM_EINVAL for a null `out` or a non-positive dimension (K = 0 is valid for the accumulating product), PM_ERANGE past
    INT32_MAX (K of the accumulating product is not limited): the conditions of pm_gemm_nt_f64 / pm_gemm_tn_acc_gated_f64."""
    from prosper_amd import _lib
    lib = _lib.load(det)
    out = (ctypes.c_int32 * 3)()
    assert lib.pm_gemm_nt_plan(128, 128, 8, 1, None) == PM_EINVAL
    assert lib.pm_gemm_tn_plan(128, 128, 8, 1, None) == PM_EINVAL
    for bad in [(0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 1, 1), (1, -5, 1), (1, 1, -1)]:
        assert lib.pm_gemm_nt_plan(*bad, 1, out) == PM_EINVAL, bad
    for bad in [(0, 1, 1), (1, 0, 1), (-1, 1, 1), (1, -5, 1), (1, 1, -1)]:
        assert lib.pm_gemm_tn_plan(*bad, 1, out) == PM_EINVAL, bad
    for big in [(INT32_MAX + 1, 1, 1), (1, INT32_MAX + 1, 1), (1, 1, INT32_MAX + 1)]:
        assert lib.pm_gemm_nt_plan(*big, 1, out) == PM_ERANGE, big
    for big in [(INT32_MAX + 1, 1, 1), (1, INT32_MAX + 1, 1)]:
        assert lib.pm_gemm_tn_plan(*big, 1, out) == PM_ERANGE, big
    assert lib.pm_gemm_nt_plan(INT32_MAX, INT32_MAX, INT32_MAX, 1, out) > 0
    mask, o = tn_plan(128, 128, 2 ** 45, 1, det)            # K far beyond int32: rows per split saturate
    assert mask & TN_DMA and o[2] == INT32_MAX
    assert tn_plan(128, 128, 0, 1, det) == (0, [slots_of(det), 0, 0])     # K = 0 launches nothing


@pytest.mark.parametrize("det", DET)
def test_slots_without_a_device_default_to_512(det):
    """2 per CU; 256 CUs (MI355X) when no device answers."""
    from conftest import has_gpu
    slots = slots_of(det)
    assert slots > 0 and slots % 2 == 0
    if not has_gpu():
        assert slots == 512


@pytest.mark.parametrize("det", DET)
@pytest.mark.parametrize("name", sorted(nt_path_cases(512)))
def test_nt_plan_one_shape_per_path(name, det):
    slots = slots_of(det)
    M, N, K, aligned, want, want_det = nt_path_cases(slots)[name]
    mask, out = nt_plan(M, N, K, aligned, det)
    assert mask == (want_det if det else want), (name, hex(mask))
    assert out[0] == slots
    if slots == 512:            # the figures of the docstring
        main_panels, nsplit = out[1], out[2]
        expect = {"main": (128, 1), "fused": (128, 1 if det else 2), "rest64": (64, 1), "split": (0, 1 if det else 16),
                  "rest": (0, 1)}.get(name, (0, 1))
        assert (main_panels, nsplit) == expect, name


def test_nt_plan_bits_are_all_reached():
    """Every PM_NT_PLAN_* bit appears in some case (the deterministic build's own bit in its library only)."""
    seen = seen_det = 0
    for M, N, K, aligned, _, _ in nt_path_cases(slots_of()).values():
        seen |= nt_plan(M, N, K, aligned)[0]
        seen_det |= nt_plan(M, N, K, aligned, det=True)[0]
    assert seen == 0x1FF
    assert seen_det == (NT_MAIN | NT_REST | NT_MT1 | NT_MT2 | NT_MT4 | NT_ALIGNED | NT_WHOLE)


def test_nt_plan_alignment_needs_even_k_and_dma_needs_k_mod_8():
    slots = slots_of()
    M = 128 * (slots // 4)
    assert nt_plan(M, 512, 8, 1)[0] & NT_MAIN
    assert nt_plan(M, 512, 8, 0)[0] == NT_MT4                    # 8-byte base: register kernel, scalar loads
    assert nt_plan(M, 512, 12, 1)[0] == NT_MT4 | NT_ALIGNED      # K % 8 != 0
    assert nt_plan(M, 512, 7, 1)[0] == NT_MT4                    # odd K: rows are not all 16-byte aligned


def test_nt_plan_split_factor_is_what_gets_launched():
    """out[2] is the number of non-empty slices: 20 K-steps asked to split 2 ways are 2 slices of 10; 17 K-steps asked to
    split 2 ways are 9 + 8."""
    if slots_of() != 512:      # (the figures below are for 256 CUs: the MI355X, and the default without a device)
        return
    assert nt_plan(200, 256, 160, 1) == (NT_REST_SPLIT | NT_ALIGNED, [512, 0, 2])
    assert nt_plan(200, 256, 136, 1) == (NT_REST_SPLIT | NT_ALIGNED, [512, 0, 2])
    # many slices of many tiles are halved, not below 4 (3392 x 256 x 1024: 54 tiles, 9 -> 4 slices), in the one launch that
    # also runs the whole rounds when there are any
    assert nt_plan(3392, 256, 1024, 1) == (NT_REST_SPLIT | NT_ALIGNED, [512, 0, 4])
    assert nt_plan(3392 + 128 * 256, 256, 1024, 1) == (NT_FUSED | NT_ALIGNED, [512, 256, 4])
    assert nt_plan(3392, 256, 1024, 1, det=True) == (NT_REST | NT_ALIGNED, [512, 0, 1])


@pytest.mark.parametrize("det", DET)
@pytest.mark.parametrize("name", sorted(tn_path_cases()))
def test_tn_plan_one_shape_per_path(name, det):
    M, N, K, aligned, want, nsplit = tn_path_cases()[name]
    mask, out = tn_plan(M, N, K, aligned, det)
    assert mask == want, (name, hex(mask))
    assert out[0] == slots_of(det) and out[1] == nsplit
    assert out[2] % 16 == 0 and out[2] * nsplit >= K - K % 8 and out[2] * (nsplit - 1) < K


def test_tn_plan_bits_are_all_reached():
    seen = 0
    for M, N, K, aligned, _, _ in tn_path_cases().values():
        seen |= tn_plan(M, N, K, aligned)[0]
    assert seen == 0x1F


def test_tn_plan_needs_even_m_and_n_for_the_aligned_kernel():
    assert tn_plan(33, 8, 5, 1)[0] == TN_REG
    assert tn_plan(34, 7, 5, 1)[0] == TN_REG
    assert tn_plan(34, 8, 5, 1)[0] == TN_REG | TN_ALIGNED
