"""The seeding kernels (seed_kernels.hip) through the C ABI, bit for bit against tests/seeding_reference.py:
``dist``, ``work`` = [B | Q], the potential S and the drawn index of three rounds per case, one case per plan cell, each
confirmed with pm_seed_plan.

Every operand and output sits inside a larger device buffer filled with a recognisable pattern (the method of
tests/test_eval_kernels_gpu.py: 16 guard rows before and after, the padding columns of every row): after a call the result is
compared, every other element of an output buffer still holds the pattern and the inputs are bit-unchanged.  Layouts of Y:
tight (rows 16-byte aligned iff D is even), an even stride with padding (16-byte loads with a ragged last one at odd D), an odd
stride and an even stride from an odd element offset (8-byte loads).

Data is continuous (no two rows tie) except where ties are the point: integer distances put t exactly on a block boundary."""
import ctypes

import numpy as np
import pytest

import seeding_reference as SR

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENT_F64 = 0x7FF8DEADBEEF0001
SENT_I64 = 0x5A5A5A5A5A5A5A5A
GUARD_ROWS = 16
LAYOUTS = ["tight", "even", "odd", "even_off1"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU box (MI355X)")
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module", params=[False, True], ids=["default", "det"])
def lib(request):
    from prosper_amd import _lib
    return _lib.load(request.param)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Emb:
    """A host matrix (or vector: one row) of float64 or int64 inside a pattern-filled device buffer."""

    def __init__(self, array, ld, dev, off=0):
        a = np.asarray(array)
        a = a[None, :] if a.ndim == 1 else a
        self.rows, self.cols = a.shape
        assert ld >= self.cols
        self.ld = ld
        self.f64 = a.dtype == np.float64
        self.sent = SENT_F64 if self.f64 else SENT_I64
        self.start = GUARD_ROWS * ld + off
        self.buf = torch.empty(self.start + (self.rows + GUARD_ROWS) * ld + 3, dtype=torch.float64 if self.f64 else torch.int64,
                               device=dev)
        self._raw().fill_(self.sent)
        if a.size:
            self.block().copy_(torch.from_numpy(np.ascontiguousarray(a)))
        self.before = self.buf.clone()

    def _raw(self, t=None):
        t = self.buf if t is None else t
        return t.view(torch.int64)

    def block(self):
        return self.buf[self.start:self.start + self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols]

    def host(self):
        return self.block().cpu().numpy()

    @property
    def addr(self):
        return self.buf.data_ptr() + 8 * self.start

    @property
    def ptr(self):
        return ctypes.c_void_p(self.addr)

    def at(self, i):
        return ctypes.c_void_p(self.addr + 8 * i)

    def unchanged(self):
        return torch.equal(self._raw(), self._raw(self.before))

    def outside_untouched(self):
        rest = self._raw().clone()
        rest[self.start:self.start + self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols] = self.sent
        return bool((rest == self.sent).all())


def _emb_Y(Y, layout, dev):
    D = Y.shape[1]
    ld = {"tight": D, "even": D + 2 - D % 2, "odd": D + 1 + D % 2, "even_off1": D + 2 - D % 2}[layout]
    e = Emb(Y, ld, dev, off=1 if layout == "even_off1" else 0)
    vec = e.addr % 16 == 0 and ld % 2 == 0
    assert vec == {"tight": D % 2 == 0, "even": True, "odd": False, "even_off1": False}[layout]
    return e


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(got, want, what):
    assert np.array_equal(_bits(got), _bits(want)), what


def _plan(lib, N, D):
    out = (ctypes.c_int32 * 8)()
    assert lib.pm_seed_plan(N, D, out) == 0
    rpb, nb, g, rpw = SR.plan(N, D)
    assert list(out)[:4] == [rpb, nb, g, rpw], (N, D, list(out))
    return rpb, nb, g, rpw


def _rounds(lib, dev, Y, layout, us, tag):
    """Rounds 0 .. len(us) - 1 through update / pick against the reference; returns the indices."""
    N, D = Y.shape
    rpb, nb, g, _ = _plan(lib, N, D)
    assert lib.pm_seed_work_len(N) == 2 * nb
    R = len(us)
    eY = _emb_Y(Y, layout, dev)
    ed = Emb(np.zeros(N), N, dev)
    ew = Emb(np.zeros(2 * nb), 2 * nb, dev)
    ep = Emb(np.zeros(R), R, dev)
    i0 = min(int(np.floor(us[0] * N)), N - 1)
    first = np.full(R, -7, dtype=np.int64)
    first[0] = i0
    ei = Emb(first, R, dev)
    dist = np.zeros(N)
    idx = [i0]
    st = _stream()
    for h in range(R):
        if h:
            rc = lib.pm_seed_pick_f64(ed.ptr, N, ew.ptr, None, 0.0, float(us[h]), ei.at(h), st)
            assert rc == 0, (tag, h, rc)
            want = SR.pick(dist, B, Q, rpb, us[h])
            got = int(ei.host()[0, h])
            assert got == want, (tag, h, got, want)
            idx.append(got)
        rc = lib.pm_seed_update_f64(eY.ptr, eY.ld, N, D, eY.ptr, eY.ld, N, ei.at(h), int(h == 0), ed.ptr, ew.ptr, ep.at(h), st)
        assert rc == 0, (tag, h, rc)
        if idx[h] >= 0:
            dist = SR.update(dist, SR.distances(Y, Y[idx[h]], g), h == 0)
            B, Q = SR.block_sums(dist, rpb)
        else:
            B, Q = np.zeros(nb), np.zeros(nb)
        _same(ed.host()[0], dist, (tag, h, "dist"))
        _same(ew.host()[0], np.concatenate([B, Q]), (tag, h, "work"))
        _same(ep.host()[0, h], Q[-1], (tag, h, "S"))
    assert ed.outside_untouched() and ew.outside_untouched() and ep.outside_untouched() and ei.outside_untouched(), tag
    assert eY.unchanged(), tag
    return idx


D_VALUES = [1, 2, 3, 33, 63, 64, 65, 128, 200, 1024, 1030]
N_VALUES = [1, 2, 63, 64, 65, 1023, 1024, 1025, 8269]


@pytest.mark.parametrize("D", D_VALUES)
def test_every_row_width(dev, lib, D):
    """Every g, the lanes-per-row edge at D = 2 / 3 and 32 / 33, a ragged last 16-byte load, leading dimensions larger than D;
    N = 65 (five blocks, the last of one row) and N = 1025 (rpb = 16: a second trip of the row loop at D > 32)."""
    for N in (65, 1025):
        rng = np.random.RandomState(1000 * D + N)
        Y = rng.normal(size=(N, D)) * 2.0
        us = rng.uniform(size=3)
        for layout in LAYOUTS:
            idx = _rounds(lib, dev, Y, layout, us, (D, N, layout))
            assert len(set(idx)) == 3


@pytest.mark.parametrize("N", N_VALUES)
def test_every_row_count(dev, lib, N):
    """rpb = 1 (N = 1), one block, a ragged last block, 1024 blocks' worth of rows and more (N = 8269: rpb = 16)."""
    for D in (3, 200):
        rng = np.random.RandomState(77 * N + D)
        Y = rng.normal(size=(N, D)) * 2.0
        R = min(3, N)
        us = rng.uniform(size=R)
        for layout in ("tight", "even"):
            idx = _rounds(lib, dev, Y, layout, us, (N, D, layout))
            assert len(set(idx)) == R


def test_second_trip_of_the_row_loop_at_one_lane_per_row(dev, lib):
    """D = 1: 256 rows per trip of a workgroup; N = 300 000 has rpb = 293."""
    N = 300000
    assert SR.plan(N, 1)[0] == 293
    rng = np.random.RandomState(12)
    Y = rng.normal(size=(N, 1))
    _rounds(lib, dev, Y, "tight", rng.uniform(size=2), "D1")


def _pick(lib, dev, dist, u, S=None, t_offset=0.0):
    N = len(dist)
    rpb, nb, _, _ = _plan(lib, N, 2)
    B, Q = SR.block_sums(dist, rpb)
    ed, ew = Emb(dist, N, dev), Emb(np.concatenate([B, Q]), 2 * nb, dev)
    eo = Emb(np.full(1, -7, dtype=np.int64), 1, dev)
    eS = Emb(np.array([0.0 if S is None else S]), 1, dev)
    rc = lib.pm_seed_pick_f64(ed.ptr, N, ew.ptr, None if S is None else eS.ptr, float(t_offset), float(u), eo.ptr, _stream())
    assert rc == 0
    got = int(eo.host()[0, 0])
    assert got == SR.pick(dist, B, Q, rpb, u, S=S, t_offset=t_offset), (N, u, S, t_offset)
    assert eo.outside_untouched() and ed.unchanged() and ew.unchanged() and eS.unchanged()
    return got, B, Q


def test_draws_at_the_edges(dev, lib):
    """t in the first block, in the last block, exactly on a block boundary, u = 0 and u = nextafter(1, 0); integer distances
    make u S exact where it has to be."""
    rng = np.random.RandomState(21)
    N = 1025                                         # rpb = 16, 65 blocks, the last of one row
    dist = rng.randint(1, 9, size=N).astype(np.float64)
    dist[:3] = 0.0
    dist[-1] = 0.0
    cum = np.cumsum(dist)
    total = cum[-1]
    got, B, Q = _pick(lib, dev, dist, 0.0)
    assert got == 3
    got, _, _ = _pick(lib, dev, dist, np.nextafter(1.0, 0.0))
    assert got == N - 2
    u = 5.0 / total                                  # (u S is within rounding of 5: the exact sums decide)
    assert _pick(lib, dev, dist, u)[0] == int(np.searchsorted(cum, u * total, side="right")) < 16
    u = (total - 3.0) / total
    assert _pick(lib, dev, dist, u)[0] == int(np.searchsorted(cum, u * total, side="right")) >= N - 17
    hit = 0
    for b in (0, 1, 31, 62):                        # (Q_63 is the total: the last block's one row has distance 0)
        u = Q[b] / total
        if u * total == Q[b]:                        # t == Q_b: the first positive row of the next block
            hit += 1
            assert _pick(lib, dev, dist, u)[0] == int(np.searchsorted(cum, Q[b], side="right")) >= 16 * (b + 1)
    assert hit
    # the several-rank form: t = u S' + t_offset with S' given on the device
    # (as an owner rank sees it: 0.5 S of the ranks before it, t past that)
    for u in rng.uniform(0.4, 1.0, size=6):
        got, _, _ = _pick(lib, dev, dist, u, S=1.5 * total, t_offset=-0.5 * total)
        assert dist[got] > 0.0
    # continuous distances: a walk that ends within rounding of its block's end
    cont = rng.uniform(0.1, 1.0, size=N)
    for u in np.concatenate([rng.uniform(size=20), [0.0, np.nextafter(1.0, 0.0)]]):
        _pick(lib, dev, cont, u)
    Bc, Qc = SR.block_sums(cont, 16)
    for b in (0, 7, 63):
        for u in (Qc[b] / Qc[-1], np.nextafter(Qc[b] / Qc[-1], 0.0), np.nextafter(Qc[b] / Qc[-1], 1.0)):
            _pick(lib, dev, cont, u)


def test_shard_of_mostly_zero_distances(dev, lib):
    rng = np.random.RandomState(22)
    N = 8269
    dist = np.zeros(N)
    where = rng.choice(N, size=9, replace=False)
    dist[where] = rng.uniform(0.5, 2.0, size=9)
    for u in np.concatenate([rng.uniform(size=12), [0.0, np.nextafter(1.0, 0.0)]]):
        got, _, _ = _pick(lib, dev, dist, u)
        assert dist[got] > 0.0
    assert _pick(lib, dev, np.zeros(N), 0.3)[0] == -1


def test_exhausted_shard_and_dead_index(dev, lib):
    """Three distinct rows, five rounds: S reaches 0 in round 2, the draws of rounds 3 and 4 are -1 and their updates leave
    dist as it is and write zeros.  Then idx = -1 and an index past the centre rows, handed over directly."""
    rng = np.random.RandomState(23)
    rows = rng.normal(size=(3, 5))
    Y = rows[rng.randint(0, 3, size=70)]
    Y[:3] = rows
    idx = _rounds(lib, dev, Y, "even", rng.uniform(size=5), "exhausted")
    assert len({tuple(Y[i]) for i in idx[:3]}) == 3 and idx[3:] == [-1, -1]
    N, D = 70, 5
    rpb, nb, g, _ = _plan(lib, N, D)
    for dead in (-1, N):
        d0 = rng.uniform(size=N)
        eY, ed = _emb_Y(Y, "tight", dev), Emb(d0, N, dev)
        ew, ep = Emb(np.ones(2 * nb), 2 * nb, dev), Emb(np.ones(1), 1, dev)
        ei = Emb(np.array([dead], dtype=np.int64), 1, dev)
        assert lib.pm_seed_update_f64(eY.ptr, eY.ld, N, D, eY.ptr, eY.ld, N, ei.ptr, 0, ed.ptr, ew.ptr, ep.ptr, _stream()) == 0
        assert ed.unchanged() and ei.unchanged() and not ew.host().any() and ep.host()[0, 0] == 0.0
        assert ew.outside_untouched() and ep.outside_untouched()


def test_centre_from_another_buffer_and_gather(dev, lib):
    """idx_dev NULL: row 0 of centre_src (the several-rank path hands over the broadcast row); pm_seed_gather_f64."""
    rng = np.random.RandomState(24)
    N, D = 333, 37
    rpb, nb, g, _ = _plan(lib, N, D)
    Y, c = rng.normal(size=(N, D)), rng.normal(size=(1, D))
    eY, ec = _emb_Y(Y, "odd", dev), Emb(c, D + 3, dev)
    ed, ew, ep = Emb(np.zeros(N), N, dev), Emb(np.zeros(2 * nb), 2 * nb, dev), Emb(np.zeros(1), 1, dev)
    assert lib.pm_seed_update_f64(eY.ptr, eY.ld, N, D, ec.ptr, ec.ld, 1, None, 1, ed.ptr, ew.ptr, ep.ptr, _stream()) == 0
    dist = SR.distances(Y, c[0], g)
    B, Q = SR.block_sums(dist, rpb)
    _same(ed.host()[0], dist, "dist")
    _same(ew.host()[0], np.concatenate([B, Q]), "work")
    _same(ep.host()[0, 0], Q[-1], "S")
    assert ed.outside_untouched() and ew.outside_untouched() and ep.outside_untouched() and eY.unchanged() and ec.unchanged()
    # potential_out NULL: S stays in work alone
    assert lib.pm_seed_update_f64(eY.ptr, eY.ld, N, D, ec.ptr, ec.ld, 1, None, 0, ed.ptr, ew.ptr, None, _stream()) == 0
    _same(ed.host()[0], dist, "dist after the same centre again")
    idx = np.array([5, -1, N - 1, 0, N, 5], dtype=np.int64)
    ei = Emb(idx, len(idx), dev)
    eo = Emb(np.full((len(idx), D), 7.5), D + 2, dev)
    assert lib.pm_seed_gather_f64(eY.ptr, eY.ld, N, D, ei.ptr, len(idx), eo.ptr, eo.ld, _stream()) == 0
    want = np.full((len(idx), D), 7.5)
    for h, i in enumerate(idx):
        if 0 <= i < N:
            want[h] = Y[i]
    _same(eo.host(), want, "gather")
    assert eo.outside_untouched() and ei.unchanged() and eY.unchanged()
