"""GPU: the ground-truth correspondences (csrc/radius.hip: correspond_row, k_correspond_rows[_batch], k_correspond_emit[_batch])
at their edges, entry for entry against the float64 brute force of oracle/correspondences.py: clouds far from the origin
(where fp32 rounding of the moved point can change its cell), a row at and above the 1024-entry staging cap, moved points
the grid rejects, K at the row lengths, and pairs whose rows share a workgroup."""
import numpy as np
import pytest
import torch

from oracle.correspondences import get_correspondences as oracle_corr
from pcrcg_amd.correspondences import _INFLATE, get_correspondences, get_correspondences_batch

from .test_correspondences_batch_gpu import RADIUS, _pairs, _rigid

pytestmark = pytest.mark.gpu

SHIFTS = (64.0, 500.0, 5000.0)
# the target grid's cells as pcrcg_cellgrid_build makes them: the radius arrives as a float, the cell is a hair wider
CELL = float(np.float32(RADIUS * _INFLATE)) * (1.0 + 1e-5)
INV_CELL = 1.0 / CELL


def _cell(x):
    """cell_coords: floor(x * inv_cell) in float64."""
    return np.floor(np.asarray(x, np.float64) * INV_CELL)


def _f32_towards(x, goal):
    """x rounded to fp32, then stepped (if the rounding went the other way) so that it lies on goal's side of x."""
    y = np.asarray(x, np.float64).astype(np.float32)
    wrong = np.sign(y.astype(np.float64) - x) == -np.sign(goal - x)
    return np.where(wrong, np.nextafter(y, np.asarray(goal, np.float32)), y).astype(np.float32)


def _far_pair(shift):
    """300/300 points in a half-metre cube moved by `shift` on every axis (the shift goes into the transform too), plus
    planted pairs, all found on the CPU among 1 500 000 candidate source points by what their float64 moved point p does:

    near : p lies within 1e-5 m below a face of the target grid's cells; its target sits 0.0374 m towards the opposite
           face.  (0.0374 + 1e-5 is less than a cell, so this target shares p's cell: the pair is found whichever of the two
           cells fp32 rounding puts p in.  It pins the candidates next to a face.)
    lost : (float)p lies in ANOTHER cell than p does, and the target lies in the cell on the far side of p's own, as close
           to the face between them as fp32 allows, and within the radius in float64.  A search that takes the cell from
           (float)p probes three cells that do not hold this target.  Such pairs need half an fp32 ulp to exceed the
           margin cell - radius = 4.1e-6 m: none exists at 64 m (half an ulp: 3.8e-6), they do at 500 m and 5000 m.
    -> src, tgt (float32), T, planted: {"near": [(i, j)], "lost": [(i, j)]}"""
    rng = np.random.RandomState(int(shift))
    T = _rigid(rng, 0.3, [0.05, -0.02, 0.03])
    R = T[:3, :3]
    s = np.full(3, shift)
    T[:3, 3] = T[:3, 3] + s - R @ s
    base = rng.rand(300, 3) * 0.5
    src = (base + s).astype(np.float32)
    tgt = ((base @ R.T + T[:3, 3] + R @ s + rng.randn(300, 3) * 0.01)[rng.permutation(300)]).astype(np.float32)
    cand = (rng.rand(1500000, 3) * 0.5 + s).astype(np.float32)
    p = cand.astype(np.float64) @ R.T + T[:3, 3]                          # as the brute force moves them
    c64 = _cell(p)
    c32 = _cell(p.astype(np.float32))
    below = (c64 + 1) * CELL - p                                          # distance to the face above, per axis
    extra_s, extra_t, planted = [], [], {"near": [], "lost": []}

    def plant(kind, row, target):
        planted[kind].append((300 + len(extra_s), 300 + len(extra_t)))
        extra_s.append(cand[row])
        extra_t.append(target)

    rows, axes = np.nonzero((below > 0) & (below < 1e-5))
    for row, a in list(zip(rows, axes))[:100]:
        want = p[row].copy()
        want[a] -= 0.0374
        target = want.astype(np.float32)
        target[a] = _f32_towards(want[a], p[row, a])
        plant("near", row, target)
    rows, axes = np.nonzero(c32 != c64)
    for row, a in zip(rows, axes):
        if len(planted["lost"]) == 100:
            break
        up = c32[row, a] > c64[row, a]                                    # rounded up: the lost cell is the one below p's
        face = (c64[row, a] if up else c64[row, a] + 1) * CELL
        x = np.float32(face)
        for _ in range(4):                                               # step off the face into the far cell
            if _cell(x) == c64[row, a] + (-1 if up else 1):
                break
            x = np.nextafter(x, np.float32(-np.inf if up else np.inf))
        target = p[row].astype(np.float32)
        target[a] = x
        if np.sqrt(((target.astype(np.float64) - p[row]) ** 2).sum()) < RADIUS and _cell(x) == c64[row, a] + (-1 if up else 1):
            plant("lost", row, target)
    if extra_s:
        src = np.concatenate([src, np.stack(extra_s)])
        tgt = np.concatenate([tgt, np.stack(extra_t)])
    return src, tgt, T, planted


@pytest.fixture(scope="module")
def far():
    """shift -> (src, tgt, T, planted, brute force), computed once."""
    out = {}
    for shift in SHIFTS:
        src, tgt, T, planted = _far_pair(shift)
        out[shift] = (src, tgt, T, planted, oracle_corr(src, tgt, T, RADIUS))
    return out


def test_the_far_cases_are_what_they_claim(far):
    for shift in SHIFTS:
        src, tgt, T, planted, brute = far[shift]
        assert np.abs(src).min() >= shift and np.abs(tgt).min() >= shift - 0.25
        have = set(map(tuple, brute.tolist()))
        assert len(brute) > 300
        assert len(planted["near"]) == 100
        assert all(pair in have for pair in planted["near"]) and all(pair in have for pair in planted["lost"])
        p = src.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
        t64 = tgt.astype(np.float64)
        for i, j in planted["near"]:
            below = (_cell(p[i]) + 1) * CELL - p[i]
            a = int(np.argmin(below))
            assert 0 < below[a] < 1e-5
            d = np.sqrt(((t64[j] - p[i]) ** 2).sum())
            assert d < RADIUS - 9e-5 and 0.0374 - 5e-4 < p[i, a] - t64[j, a] <= 0.0374          # (fp32 steps of 4.9e-4 at 5000 m)
        for i, j in planted["lost"]:
            # the 27 cells around the cell of (float)p do not hold the target; the 27 around p's own do
            assert np.abs(_cell(t64[j]) - _cell(p[i].astype(np.float32))).max() == 2
            assert np.abs(_cell(t64[j]) - _cell(p[i])).max() == 1
            assert np.sqrt(((t64[j] - p[i]) ** 2).sum()) < RADIUS
        print(f"shift {shift}: {len(planted['near'])} near, {len(planted['lost'])} lost pairs planted, {len(brute)} pairs in all")
    assert len(far[64.0][3]["lost"]) == 0              # half an fp32 ulp at 64 m is below the cell's margin
    assert len(far[500.0][3]["lost"]) >= 10 and len(far[5000.0][3]["lost"]) == 100


def _missing(got, brute):
    have = set(map(tuple, got.tolist()))
    return [pair for pair in map(tuple, brute.tolist()) if pair not in have]


@pytest.mark.parametrize("shift", SHIFTS)
def test_far_from_the_origin_single_call(cuda, far, shift):
    src, tgt, T, planted, brute = far[shift]
    got = get_correspondences(torch.from_numpy(src).to(cuda), torch.from_numpy(tgt).to(cuda), T, RADIUS).cpu().numpy()
    lost = _missing(got, brute)
    print(f"shift {shift}: {len(got)} pairs, brute force {len(brute)}, missing {len(lost)} "
          f"({len(set(lost) & set(planted['lost']))} of them planted): {lost[:4]}")
    assert np.array_equal(got, brute)


def test_far_from_the_origin_batch_call(cuda, far):
    near = _pairs()[3]
    items = [far[s][:3] for s in SHIFTS] + [near]
    want = [far[s][4] for s in SHIFTS] + [oracle_corr(*near, RADIUS)]
    got = get_correspondences_batch([torch.from_numpy(s).to(cuda) for s, _, _ in items],
                                    [torch.from_numpy(t).to(cuda) for _, t, _ in items], [T for _, _, T in items], RADIUS)
    for b in range(4):
        g = got[b].cpu().numpy()
        print(f"pair {b}: {len(g)} pairs, brute force {len(want[b])}, missing {len(_missing(g, want[b]))}")
    for b in range(4):
        assert np.array_equal(got[b].cpu().numpy(), want[b]), b


def _ball(rng, count, r_lo, r_hi):
    v = rng.randn(count, 3)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return v * rng.uniform(r_lo, r_hi, (count, 1))


def _crowded(count):
    """One source point with `count` targets within the radius (and 40 outside it), under a small rigid transform."""
    rng = np.random.RandomState(count)
    T = _rigid(rng, 0.2, [0.02, 0.01, -0.03])
    src = np.array([[0.25, 0.125, 0.375]], np.float32)
    p = src.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    tgt = np.concatenate([p + _ball(rng, count, 0.001, 0.036), p + _ball(rng, 40, 0.039, 0.07)])
    return src, tgt[rng.permutation(len(tgt))].astype(np.float32), T


def test_a_row_at_and_above_the_staging_cap(cuda):
    ordinary = [_pairs()[2], _pairs()[3]]
    want = [oracle_corr(s, t, T, RADIUS) for s, t, T in ordinary]
    dev = lambda items: ([torch.from_numpy(s).to(cuda) for s, _, _ in items], [torch.from_numpy(t).to(cuda) for _, t, _ in items],
                         [T for _, _, T in items])
    over, full = _crowded(1100), _crowded(1024)
    b_over, b_full = oracle_corr(*over, RADIUS), oracle_corr(*full, RADIUS)
    assert len(b_over) == 1100 and len(b_full) == 1024 and (b_full[:, 0] == 0).all()      # the rows are what they claim
    for items in ([ordinary[0], over, ordinary[1]],):
        s, t, Ts = dev(items)
        with pytest.raises(RuntimeError, match=r"has 1100 targets within the radius \(more than the 1024"):
            get_correspondences_batch(s, t, Ts, RADIUS)
        with pytest.raises(RuntimeError, match=r"has 1100 targets within the radius \(more than the 1024"):
            get_correspondences(s[1], t[1], Ts[1], RADIUS)
        # the same stream is still good: an ordinary call, then the full row
        assert np.array_equal(get_correspondences(s[0], t[0], Ts[0], RADIUS).cpu().numpy(), want[0])
    s, t, Ts = dev([ordinary[0], full, ordinary[1]])
    got = get_correspondences_batch(s, t, Ts, RADIUS)
    assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[2].cpu().numpy(), want[1])
    assert np.array_equal(got[1].cpu().numpy(), b_full)
    assert np.array_equal(get_correspondences(s[1], t[1], Ts[1], RADIUS).cpu().numpy(), b_full)
    assert np.array_equal(get_correspondences_batch(s, t, Ts, RADIUS, K=1000)[1].cpu().numpy(), b_full[:1000])


def test_rows_whose_moved_point_the_grid_rejects(cuda):
    pairs = [_pairs()[2], _pairs()[3], _pairs()[2]]
    src = [torch.from_numpy(s).to(cuda) for s, _, _ in pairs]
    tgt = [torch.from_numpy(t).to(cuda) for _, t, _ in pairs]
    want = [oracle_corr(s, t, T, RADIUS) for s, t, T in pairs]
    far_T = pairs[1][2].copy()
    far_T[:3, 3] = 1e9
    assert len(oracle_corr(pairs[1][0], pairs[1][1], far_T, RADIUS)) == 0
    nan_T = pairs[1][2].copy()
    nan_T[1, 1] = np.nan
    for bad in (far_T, nan_T):
        got = get_correspondences_batch(src, tgt, [pairs[0][2], bad, pairs[2][2]], RADIUS)
        assert tuple(got[1].shape) == (0, 2) and got[1].dtype == torch.int64
        assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[2].cpu().numpy(), want[2])
        assert tuple(get_correspondences(src[1], tgt[1], bad, RADIUS).shape) == (0, 2)
    assert len(want[0]) > 1000 and len(want[1]) > 10000


def test_keep_at_the_longest_row(cuda):
    s, t, T = _pairs()[3]
    full = oracle_corr(s, t, T, RADIUS)
    longest = int(np.bincount(full[:, 0]).max())
    assert 32 < longest <= 1024
    src, tgt = torch.from_numpy(s).to(cuda), torch.from_numpy(t).to(cuda)
    for K in (1, longest, longest + 1):
        want = oracle_corr(s, t, T, RADIUS, K=K)
        assert np.array_equal(get_correspondences(src, tgt, T, RADIUS, K=K).cpu().numpy(), want), K
        got = get_correspondences_batch([src, src], [tgt, tgt], [T, T], RADIUS, K=K)
        assert np.array_equal(got[0].cpu().numpy(), want) and np.array_equal(got[1].cpu().numpy(), want), K
        if K >= longest:
            assert np.array_equal(want, full)
        else:
            assert len(want) == len(np.unique(full[:, 0]))


LENGTHS = (1, 3, 4, 5, 259)


def _short_pairs():
    """Pairs of 1, 3, 4, 5 and 259 source rows: a workgroup holds four wavefronts of one row each, so rows 0..3 of the batch
    belong to two pairs, rows 4..7 to two, rows 8..11 to two and rows 12..15 to two.  Every pair has its own transform, and
    every source row has the target that is its own image (and the 259-row pair more)."""
    rng = np.random.RandomState(77)
    out = []
    for k, n in enumerate(LENGTHS):
        T = _rigid(rng, 0.1 * (k + 1), rng.rand(3) * 0.1)
        src = (rng.rand(n, 3) * 0.2).astype(np.float32)
        img = src.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
        tgt = np.concatenate([img + rng.randn(n, 3) * 0.002, rng.rand(20, 3) * 0.3])
        out.append((src, tgt[rng.permutation(len(tgt))].astype(np.float32), T))
    return out


def test_pair_boundaries_inside_a_workgroup(cuda):
    pairs = _short_pairs()
    want = [oracle_corr(s, t, T, RADIUS) for s, t, T in pairs]
    for (s, _, _), w in zip(pairs, want):
        assert w[0, 0] == 0 and w[-1, 0] == len(s) - 1                   # the first and the last row of every pair have pairs
    starts = np.cumsum([0] + list(LENGTHS))
    assert any(starts[b] // 4 == (starts[b + 1] - 1) // 4 == starts[b + 1] // 4 for b in range(3))    # a workgroup spans pairs
    for order in ([0, 1, 2, 3, 4], [4, 3, 2, 1, 0], [1, 4, 0, 2, 3]):
        got = get_correspondences_batch([torch.from_numpy(pairs[b][0]).to(cuda) for b in order],
                                        [torch.from_numpy(pairs[b][1]).to(cuda) for b in order],
                                        [pairs[b][2] for b in order], RADIUS)
        for pos, b in enumerate(order):
            g = got[pos].cpu().numpy()
            assert np.array_equal(g, want[b]), (order, b)
            assert g[:, 0].min() == 0 and g[:, 0].max() == LENGTHS[b] - 1
