"""Numpy restatements of pcrcg_voxel_down_sample_batch (include/pcrcg.h "Voxel down-sampling") and the
inputs its tests share.  Two restatements of one definition: a vectorised one (the tests' reference) and a literal
dict-and-loop one; tests/test_voxel_cpu.py holds them to the same bits.

Per cloud, every step in float64 from the exactly widened fp32 coordinates:
    vmin = min - 0.5 * voxel;  idx = (int)floor((p - vmin) / voxel);  equal idx = one voxel;
    row = (sum of the voxel's points, one by one in ascending input index, from 0.0) / (double)count;
    rows in ascending index of each voxel's first input point.
A cloud with a non-finite coordinate, or with an index that would reach 2^21, is rejected (None)."""
import numpy as np

INDEX_LIMIT = 1 << 21


def _frame(pts, voxel):
    """-> (p64, idx [N,3] int64) or None for a rejected cloud."""
    pts = np.asarray(pts, dtype=np.float32).reshape(-1, 3)
    if not np.isfinite(pts).all():
        return None
    p64 = pts.astype(np.float64)
    voxel = np.float64(voxel)
    vmin = p64.min(0) - np.float64(0.5) * voxel
    q = np.floor((p64 - vmin) / voxel)
    if not (q < INDEX_LIMIT).all():
        return None
    return p64, q.astype(np.int64)


def voxel_down_sample(pts, voxel):
    """Vectorised restatement -> (rows [K,3] float64, first [K] int32, count [K] int32), or None for a rejected cloud."""
    pts = np.asarray(pts, dtype=np.float32).reshape(-1, 3)
    if len(pts) == 0:
        return np.zeros((0, 3), np.float64), np.zeros(0, np.int32), np.zeros(0, np.int32)
    fr = _frame(pts, voxel)
    if fr is None:
        return None
    p64, idx = fr
    key = idx[:, 0] | (idx[:, 1] << 21) | (idx[:, 2] << 42)
    _, first, inverse = np.unique(key, return_index=True, return_inverse=True)   # first: lowest input row of every voxel
    order = np.argsort(first, kind="stable")                                     # voxels by their first input row
    place = np.empty_like(order)
    place[order] = np.arange(len(order))
    row_of = place[inverse.reshape(-1)]
    sums = np.zeros((len(order), 3), np.float64)
    np.add.at(sums, row_of, p64)              # unbuffered: the points are added one by one in input order
    count = np.bincount(row_of, minlength=len(order))
    return sums / count[:, None].astype(np.float64), first[order].astype(np.int32), count.astype(np.int32)


def voxel_down_sample_literal(pts, voxel):
    """The definition word for word: a dict from index triple to [sum, count, first], filled in one pass over the points."""
    pts = np.asarray(pts, dtype=np.float32).reshape(-1, 3)
    voxel = np.float64(voxel)
    for p in pts:
        for v in p:
            if not np.isfinite(v):
                return None
    cells = {}
    if len(pts):
        vmin = [np.float64(min(np.float64(p[d]) for p in pts)) - np.float64(0.5) * voxel for d in range(3)]
    for i, p in enumerate(pts):
        q = [np.floor((np.float64(p[d]) - vmin[d]) / voxel) for d in range(3)]
        if any(not (v < INDEX_LIMIT) for v in q):
            return None
        cell = cells.setdefault(tuple(int(v) for v in q), [[np.float64(0.0)] * 3, 0, i])
        cell[0] = [cell[0][d] + np.float64(p[d]) for d in range(3)]
        cell[1] += 1
    rows = sorted(cells.values(), key=lambda c: c[2])
    out = np.array([[c[0][d] / np.float64(c[1]) for d in range(3)] for c in rows], np.float64).reshape(-1, 3)
    return out, np.array([c[2] for c in rows], np.int32), np.array([c[1] for c in rows], np.int32)


# ---- inputs ---------------------------------------------------------------------------------------------------------
def cube(seed, n, side=3.0, shift=0.0):
    """n random fp32 points in a cube of `side` metres, moved by `shift` along every axis."""
    return (np.random.RandomState(seed).rand(n, 3) * side + shift).astype(np.float32)


def own_voxels(n, voxel=0.3):
    """n points, each in a voxel of its own: a shuffled lattice with a pitch of two voxels (hash-table load)."""
    rng = np.random.RandomState(n)
    side = int(np.ceil(n ** (1 / 3)))
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)[:n]
    return (rng.permutation(g) * (2 * voxel) + rng.rand(n, 3) * 0.1 * voxel).astype(np.float32)


def one_voxel(n, voxel=0.3):
    """n distinct points inside one voxel (the ordered sum of one long list)."""
    return (5.0 + np.random.RandomState(n).rand(n, 3) * 0.4 * voxel).astype(np.float32)


def duplicates(seed=3, n=300, copies=4):
    """Every point `copies` times, shuffled."""
    p = np.repeat(cube(seed, n), copies, 0)
    return p[np.random.RandomState(seed).permutation(len(p))]


def on_faces(voxel=0.25, lo=-2.0, k=17):
    """Points exactly on voxel faces: min + (j + 0.5) * voxel for a power-of-two voxel, so (p - vmin) / voxel is the exact
    integer j + 1, on both sides of zero; plus the points one fp32 step below and above every face."""
    c = (lo + (np.arange(k) + 0.5) * voxel).astype(np.float32)
    assert (c.astype(np.float64) == lo + (np.arange(k) + 0.5) * voxel).all() and c.min() < 0 < c.max()
    c = np.concatenate([[np.float32(lo)], c, np.nextafter(c, np.float32(-np.inf)), np.nextafter(c, np.float32(np.inf))])
    rng = np.random.RandomState(5)
    return np.stack([rng.permutation(c), rng.permutation(c), rng.permutation(c)], 1).astype(np.float32)


def slab(seed, n):
    """A KITTI-shaped slab (40 m x 40 m x 0.6 m) of n fp32 points."""
    return (np.random.RandomState(seed).rand(n, 3) * np.array([40.0, 40.0, 0.6])).astype(np.float32)


def too_fine(voxel=0.3):
    """Two points whose distance over the voxel size reaches 2^21 on x: rejected."""
    return np.array([[0.0, 0.0, 0.0], [voxel * (INDEX_LIMIT + 8), 1.0, 1.0]], np.float32)


def single_cases(voxel=0.3):
    """name -> (points, voxel): every single-cloud case of tests/test_voxel_gpu.py (and of the CPU agreement test)."""
    cases = {f"n{n}": (cube(10 + n, n), voxel) for n in (0, 1, 2, 255, 256, 257, 1023, 1025)}
    cases["own_voxels_5000"] = (own_voxels(5000, voxel), voxel)
    cases["one_voxel_1500"] = (one_voxel(1500, voxel), voxel)
    cases["duplicates"] = (duplicates(), voxel)
    cases["faces"] = (on_faces(), 0.25)
    cases["cube_plus_1000m"] = (cube(21, 600, shift=1000.0), voxel)
    cases["cube_minus_1000m"] = (cube(22, 600, shift=-1000.0), voxel)
    return cases
