"""The deterministic-mode audit (tests/det_audit.py) catches the faults it is for: an accumulator emulated in NumPy -- 700
random addends in three categories -- once correct and three times with a planted fault, plus PM_Q's rounding against integer
arithmetic on the mantissa.  No GPU, no library."""
import numpy as np
import pytest

import det_audit as A

N_ADD = 700
BOUNDS = (700.0, 700.0 * 40.0, 700.0 * 9.0)          # sums of probabilities | of energies | of log-evidences
UP = {c: 12 + 4 * c for c in range(5)}               # the two orders of coarse, distinct quanta the GPU audit runs
DOWN = {c: 12 + 4 * (4 - c) for c in range(5)}
SLOTS = 24


def _addends():
    rng = np.random.RandomState(3)
    return [rng.uniform(0.0, 1.0, size=(N_ADD, SLOTS)),              # category 0: probabilities
            rng.uniform(0.0, 40.0, size=(N_ADD, SLOTS)),             # category 1: q e
            rng.normal(scale=3.0, size=(N_ADD, SLOTS))]              # category 2: signed


def _accumulate(shifts, cat_used=(0, 1, 2), skip=None):
    """Three blocks; block b sums its addends after pm_q with category cat_used[b]'s magic constant, in a shuffled order;
    `skip` = (block, addend): that one goes in unrounded.  Returns the blocks and the quanta their OWN categories have."""
    magics = [A.magic_of(BOUNDS[c] * 2.0 ** shifts[c]) for c in range(3)]
    rng = np.random.RandomState(4)
    out = []
    for b, v in enumerate(_addends()):
        v = v[rng.permutation(N_ADD)]
        r = A.pm_q(v, magics[cat_used[b]])
        if skip is not None and skip[0] == b:
            r[skip[1]] = v[skip[1]]
        acc = np.zeros(SLOTS)
        for row in r:
            acc += row
        out.append(acc)
    return out, [A.quantum(m) for m in magics]


def _complaints(blocks, quanta):
    bad = []
    for b, (x, q) in enumerate(zip(blocks, quanta)):
        bad += A.check_block("block%d" % b, x, q)
    return bad


@pytest.mark.parametrize("shifts", [UP, DOWN], ids=["ascending", "descending"])
def test_correct_accumulator_passes_and_is_order_independent(shifts):
    blocks, quanta = _accumulate(shifts)
    assert _complaints(blocks, quanta) == []
    magics = [A.magic_of(BOUNDS[c] * 2.0 ** shifts[c]) for c in range(3)]
    for b, v in enumerate(_addends()):           # any other order: the same bits (what the mode promises)
        assert np.array_equal(A.pm_q(v, magics[b])[::-1].cumsum(axis=0)[-1], blocks[b])
        assert np.abs(blocks[b] - v.astype(np.longdouble).sum(axis=0)).max() <= N_ADD * quanta[b] / 2


def test_one_unrounded_addend_is_caught():
    blocks, quanta = _accumulate(UP, skip=(1, 123))
    bad = _complaints(blocks, quanta)
    assert len(bad) == 1 and bad[0].startswith("block1:") and "no multiple" in bad[0], bad


def test_a_finer_neighbours_category_is_caught_under_ascending_shifts():
    blocks, quanta = _accumulate(UP, cat_used=(0, 0, 2))          # block 1 rounded with category 0's (finer) quantum
    assert quanta[0] < quanta[1]
    bad = _complaints(blocks, quanta)
    assert len(bad) == 1 and bad[0].startswith("block1:") and "no multiple" in bad[0], bad


def test_a_coarser_neighbours_category_needs_the_descending_order():
    blocks, quanta = _accumulate(UP, cat_used=(0, 2, 2))          # block 1 rounded with category 2's quantum: coarser here,
    assert quanta[2] > quanta[1]                                  # every multiple of it is one of block 1's own
    assert _complaints(blocks, quanta) == []
    blocks, quanta = _accumulate(DOWN, cat_used=(0, 2, 2))        # ... and finer in the other order
    assert quanta[2] < quanta[1]
    bad = _complaints(blocks, quanta)
    assert len(bad) == 1 and bad[0].startswith("block1:") and "no multiple" in bad[0], bad


def test_vacuous_blocks_fail():
    q = 2.0 ** -20
    assert any("all zero" in s for s in A.check_block("z", np.zeros(5), q))
    assert any("vacuous" in s for s in A.check_block("tiny", np.array([3 * q, 5 * q, 64 * q]), q))
    assert A.check_block("ok", np.array([0.0, 3 * q, 64 * q, 1000 * q]), q) == []
    assert A.check_block("none", np.ones(3), None) != []


def _round_by_integers(v, e):
    """Nearest multiple of q = 2^(e-52), ties to even, in Python integers: v = m 2^x exactly -> m 2^(x - (e-52)) as a
    fraction."""
    import fractions
    r = fractions.Fraction(float(v)) / fractions.Fraction(2) ** (e - 52)
    fl = r.numerator // r.denominator
    rem = r - fl
    k = fl + (1 if (rem > fractions.Fraction(1, 2) or (rem == fractions.Fraction(1, 2) and fl % 2 == 1)) else 0)
    return float(k * fractions.Fraction(2) ** (e - 52))


@pytest.mark.parametrize("e", [-3, 0, 11, 40])
def test_pm_q_against_integer_arithmetic(e):
    magic = 1.5 * 2.0 ** e
    q = A.quantum(magic)
    assert q == 2.0 ** (e - 52) and A.quantum(0.0) is None
    assert A.magic_of(2.0 ** (e - 1)) == magic and A.magic_of(2.0 ** (e - 1) * 1.0000001) == 2 * magic and A.magic_of(0.0) == 0.0
    rng = np.random.RandomState(e + 10)
    edge = [0.5 * q, 1.5 * q, 2.5 * q, -0.5 * q, -1.5 * q, 2.0 ** (e - 1) - q, -(2.0 ** (e - 1) - q), 0.0, q, 0.49999 * q,
            0.50001 * q, 2.0 ** (e - 1) - 1.5 * q]
    vals = np.concatenate([edge, rng.uniform(-1, 1, size=300) * 2.0 ** (e - 1), rng.uniform(-40, 40, size=100) * q])
    got = A.pm_q(vals, magic)
    want = np.array([_round_by_integers(v, e) for v in vals])
    assert np.array_equal(got, want)
    assert got[0] == 0.0 and got[1] == 2 * q and got[2] == 2 * q            # ties go to the even multiple
    assert got[5] == 2.0 ** (e - 1) - q                                       # the largest addend the bound allows: exact
    assert A.is_multiple(got, q).all() and not A.is_multiple(0.5 * q, q) and A.is_multiple(-3 * q, q)


@pytest.mark.parametrize("descending", [False, True])
def test_aligned_shifts_put_the_quanta_two_bits_apart_in_the_requested_order(descending):
    bounds = [700.0, 700.0 * 4.1e4, 700.0 * 350.0, 3.0, 9.9e9]            # magnitudes all over the place
    sh = A.aligned_shifts(descending)("unit", bounds)
    q = [np.log2(A.quantum(A.magic_of(b * 2.0 ** k))) for b, k in zip(bounds, sh)]
    assert list(np.diff(q)) == [-2.0 if descending else 2.0] * 4 and min(sh) >= 2
