"""NumPy restatement of the k-means++ seeding kernels (include/prosper_hip.h, seed_kernels.hip), operation for
operation: every sum is a chain of float64 additions in the documented order, every product and difference is rounded once
(NumPy never fuses).  ``rpb`` and ``g`` are arguments so that a test hands over what pm_seed_plan reported; ``plan`` is the
documented rule.  Loops run over the summation order; where rows are independent of one another they are vectorised over
rows, which changes no bit.  Not a test module."""
import numpy as np


def plan(N, D):
    """(rpb, nb, g, rows per wavefront): rpb = ceil(N / min(1024, ceil(N / 16))), nb = ceil(N / rpb), g the smallest power of
    two >= min(D, 64), a row on max(g / 2, 1) lanes."""
    nb = min(1024, -(-N // 16))
    rpb = -(-N // nb)
    g = 1
    while g < min(D, 64):
        g *= 2
    return rpb, -(-N // rpb), g, 64 // max(g // 2, 1)


def work_len(N):
    return 2 * max(plan(N, 1)[1], 1) if N > 0 else 2


def distances(Y, c, g):
    """(N,) squared distances of the rows of Y to c in the kernel's order."""
    Y = np.asarray(Y, dtype=np.float64)
    N, D = Y.shape
    part = np.zeros((N, g))
    for d in range(D):                      # ascending d: partial sum d % g receives its terms in ascending order
        t = Y[:, d] - c[d]
        part[:, d % g] = part[:, d % g] + t * t
    o = g // 2
    while o >= 1:
        part = part + part[:, np.arange(g) ^ o]
        o //= 2
    return part[:, 0].copy()


def update(dist, dn, first):
    """dist <- dn (first) or the smaller of the two by the kernel's compare: dn < dist ? dn : dist."""
    if first:
        return dn.copy()
    return np.where(dn < dist, dn, dist)


def block_sums(dist, rpb):
    """(B, Q): B_b the block's distances added in ascending n from +0; Q_b = ((B_0 + B_1) + ...) + B_b."""
    N = len(dist)
    nb = -(-N // rpb)
    B = np.zeros(nb)
    for b in range(nb):
        acc = 0.0
        for x in dist[b * rpb:min(N, (b + 1) * rpb)]:
            acc = acc + x
        B[b] = acc
    Q = np.zeros(nb)
    q = B[0]
    Q[0] = q
    for b in range(1, nb):
        q = q + B[b]
        Q[b] = q
    return B, Q


def pick(dist, B, Q, rpb, u, S=None, t_offset=0.0):
    """pm_seed_pick_f64: the drawn row, or -1.  t = u S + t_offset with S the shard's own total unless given."""
    N = len(dist)
    own = Q[-1]
    if own == 0.0:
        return -1
    t = np.float64(u) * np.float64(own if S is None else S) + np.float64(t_offset)
    over = np.nonzero(Q > t)[0]
    if len(over):
        b = int(over[0])
    else:
        pos = np.nonzero(B > 0.0)[0]
        if not len(pos):
            return -1
        b = int(pos[-1])
    r = Q[b - 1] if b > 0 else 0.0
    last = -1
    for n in range(b * rpb, min(N, (b + 1) * rpb)):
        d = dist[n]
        r = r + d
        if d > 0.0:
            last = n
        if r > t:
            return n
    return last


def kmeanspp(shards, H, u, rpbs=None, gs=None):
    """The whole seeding over the ranks' shards (a list; one entry: one rank).  Returns (centres (H, D), global indices (H,),
    potential (H,), per-round state of rank 0's last round: (dist, B, Q))."""
    shards = [np.asarray(s, dtype=np.float64) for s in shards]
    R = len(shards)
    counts = [len(s) for s in shards]
    N, D = sum(counts), shards[0].shape[1]
    starts = np.concatenate([[0], np.cumsum(counts)])
    rpbs = rpbs or [plan(c, D)[0] if c else 0 for c in counts]
    g = (gs or [plan(1, D)[2]])[0]
    dist = [np.zeros(c) for c in counts]
    BQ = [(np.zeros(1), np.zeros(1))] * R
    sums = [0.0] * R
    centres = np.zeros((H, D))
    indices = np.full(H, -1, dtype=np.int64)
    potential = np.zeros(H)
    for h in range(H):
        owner, local = -1, -1
        if h == 0:
            i0 = min(int(np.floor(np.float64(u[0]) * N)), N - 1)
            owner = int(np.searchsorted(starts[1:], i0, side="right"))
            local = i0 - int(starts[owner])
        else:
            total = 0.0
            for s in sums:
                total = total + s
            if total != 0.0:
                t = np.float64(u[h]) * np.float64(total)
                run, before = 0.0, 0.0
                for r in range(R):
                    before = run
                    run = run + sums[r]
                    if run > t:
                        owner = r
                        break
                if owner < 0:
                    positive = [r for r in range(R) if sums[r] > 0.0]
                    if positive:
                        owner = positive[-1]
                        before = 0.0
                        for s in sums[:owner]:
                            before = before + s
                if owner >= 0:
                    B, Q = BQ[owner]
                    if R == 1:
                        local = pick(dist[0], B, Q, rpbs[0], u[h])
                    else:
                        local = pick(dist[owner], B, Q, rpbs[owner], u[h], S=total, t_offset=-before)
        if owner >= 0 and local >= 0:
            indices[h] = starts[owner] + local
            centres[h] = shards[owner][local]
            for r in range(R):
                if counts[r]:
                    dist[r] = update(dist[r], distances(shards[r], centres[h], g), h == 0)
                    BQ[r] = block_sums(dist[r], rpbs[r])
                    sums[r] = float(BQ[r][1][-1])
        else:
            for r in range(R):
                BQ[r] = (np.zeros_like(BQ[r][0]), np.zeros_like(BQ[r][1]))
                sums[r] = 0.0
        total = 0.0
        for s in sums:
            total = total + s
        potential[h] = total
    return centres, indices, potential, (dist[0], BQ[0][0], BQ[0][1])
