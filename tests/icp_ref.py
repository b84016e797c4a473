"""numpy restatement of the ICP refinement (include/pcrcg.h "ICP refinement"), step by step, for
tests/test_icp_*.py.  The product never imports this file."""
import numpy as np

from . import ransac_ref as RR

EPS32 = 2.0 ** -24          # unit roundoff of fp32
COORD_BIAS = 1 << 20        # csrc/cellgrid.h kCoordBias: cell_coords accepts |floor(x / cell)| < COORD_BIAS - 2


def grid_cell(d):
    """The cell of the target grid refine_batch builds for the distance d (pcrcg_cellgrid_build takes a float radius)."""
    return float(np.float32(d)) * (1.0 + 1e-5)


def grid_rejects(p, d):
    """cell_coords on moved points p [n,3] -> [n] bool: True where the point has no cell (far away or not finite)."""
    f = np.floor(np.asarray(p, np.float64) * (1.0 / grid_cell(d)))
    return ~((f > -(COORD_BIAS - 2)) & (f < COORD_BIAS - 2)).all(1)


def xf32(T):
    """R (row-major) then t of a float64 [4,4], rounded to fp32: what the kernel moves the points with."""
    T = np.asarray(T, np.float64)
    return np.concatenate([T[:3, :3].reshape(-1), T[:3, 3]]).astype(np.float32)


def move(src, T):
    """The source points under T: fp32, unfused, ((r0 x + r1 y) + r2 z) + t0 -> float32 [n,3]."""
    X = xf32(T)
    x, y, z = src[:, 0], src[:, 1], src[:, 2]
    return np.stack([((X[0] * x + X[1] * y) + X[2] * z) + X[9],
                     ((X[3] * x + X[4] * y) + X[5] * z) + X[10],
                     ((X[6] * x + X[7] * y) + X[8] * z) + X[11]], 1).astype(np.float32)


def evaluate(src, tgt, T, d):
    """Evaluate(T) by brute force -> (corr [n] int64: the target of every source row or -1, d2 [n] float32 of the nearest
    target, count, float64 sum).  fp32 distances ((dx dx + dy dy) + dz dz); among equal d2 the lowest target index
    (np.argmin returns the first minimum); a correspondence iff d2 < (float)(d * d)."""
    n = len(src)
    corr = np.full(n, -1, np.int64)
    best = np.full(n, np.inf, np.float32)
    if n == 0 or len(tgt) == 0 or not np.isfinite(np.asarray(T, np.float64)).all():
        return corr, best, 0, 0.0
    p = move(src, T)
    for a in range(0, n, 512):
        dx = tgt[None, :, 0] - p[a:a + 512, None, 0]
        dy = tgt[None, :, 1] - p[a:a + 512, None, 1]
        dz = tgt[None, :, 2] - p[a:a + 512, None, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        j = d2.argmin(1)
        best[a:a + 512] = d2[np.arange(len(j)), j]
        corr[a:a + 512] = j
    hit = best < np.float32(float(d) * float(d))
    corr[~hit] = -1
    return corr, best, int(hit.sum()), float(best[hit].astype(np.float64).sum())


def statistics(count, total, n):
    """(fitness, rmse) of an evaluation."""
    return (count / n if n > 0 else 0.0), (float(np.sqrt(total / count)) if count > 0 else 0.0)


def update(src, tgt, T, corr):
    """The float64 Kabsch step from the correspondences of Evaluate(T): -> (delta [4,4] or None when count < 3 or the fit is
    degenerate, sigma_2 <= 1e-12 sigma_1; singular values).  The moved points enter as the float64 values of the fp32
    results; the fit is np.linalg.svd's (ransac_ref.kabsch)."""
    hit = corr >= 0
    if hit.sum() < 3:
        return None, None
    p = move(src, T)[hit].astype(np.float64)
    q = tgt[corr[hit]].astype(np.float64)
    R, t, S = RR.kabsch(p, q)
    if S[0] == 0 or not S[1] > 1e-12 * S[0]:
        return None, S
    delta = np.eye(4)
    delta[:3, :3], delta[:3, 3] = R, t
    return delta, S


def raw_sum_update(src, tgt, T, corr):
    """k_icp_update's formula in float64 numpy (not its summation order): the sums of p, q and p q^T over the correspondences,
    cs = sum p / n, ct = sum q / n, H = sum p q^T - (sum p) ct^T with a difference within 1e-12 of its two magnitudes set to
    0, then the fit from H (np.linalg.svd) and t = ct - R cs -> delta [4,4] float64."""
    hit = corr >= 0
    n = float(hit.sum())
    p = move(src, T)[hit].astype(np.float64)
    q = tgt[corr[hit]].astype(np.float64)
    sp, sq = p.sum(0), q.sum(0)
    spq = (p[:, :, None] * q[:, None, :]).sum(0)
    cs, ct = sp / n, sq / n
    sc = np.outer(sp, ct)
    h = spq - sc
    H = np.where(np.abs(h) <= 1e-12 * (np.abs(spq) + np.abs(sc)), 0.0, h)
    U, S, Vt = np.linalg.svd(H)
    sign = np.sign(np.linalg.det(Vt.T @ U.T)) or 1.0
    R = Vt.T @ np.diag([1.0, 1.0, sign]) @ U.T
    delta = np.eye(4)
    delta[:3, :3], delta[:3, 3] = R, ct - R @ cs
    return delta


def centred_update_longdouble(src, tgt, T, corr):
    """The same step as a centred fit in np.longdouble (ransac_ref.jacobi_fit: centroids first, H from the centred points)
    -> delta [4,4] np.longdouble."""
    hit = corr >= 0
    R, t, _, ok = RR.jacobi_fit(move(src, T)[hit], tgt[corr[hit]], np.longdouble)
    assert ok
    delta = np.eye(4, dtype=np.longdouble)
    delta[:3, :3], delta[:3, 3] = R, t
    return delta


def converged(fit, rmse, fit_prev, rmse_prev, relative_fitness=1e-6, relative_rmse=1e-6):
    """open3d's test: absolute differences against the two bounds."""
    return abs(fit - fit_prev) < relative_fitness and abs(rmse - rmse_prev) < relative_rmse


def icp(src, tgt, T0, d, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6):
    """The whole loop -> (T, fitness, rmse, count, iterations, history): history[k] = (T_k, fitness_k, rmse_k)."""
    n = len(src)
    T = np.array(T0, np.float64)
    if not np.isfinite(T).all():
        return np.full((4, 4), np.nan), np.nan, np.nan, -1, -1, []
    corr, _, count, total = evaluate(src, tgt, T, d)
    fit, rmse = statistics(count, total, n)
    history = [(T.copy(), fit, rmse)]
    k = 0
    while k < max_iteration:
        delta, _ = update(src, tgt, T, corr)
        if delta is None:
            break
        T = delta @ T
        k += 1
        corr, _, count, total = evaluate(src, tgt, T, d)
        fit_prev, rmse_prev = fit, rmse
        fit, rmse = statistics(count, total, n)
        history.append((T.copy(), fit, rmse))
        if converged(fit, rmse, fit_prev, rmse_prev, relative_fitness, relative_rmse):
            break
    return T, fit, rmse, count, k, history


def stop_iteration(counts, sums, n, can_update, max_iteration, relative_fitness=1e-6, relative_rmse=1e-6):
    """The loop's control flow alone, fed with a recorded sequence of evaluations (counts[k], sums[k] of Evaluate(T_k)) and
    can_update(k) -> bool (count >= 3 and a fit that is not degenerate): the k at which the loop ends."""
    fit_prev = rmse_prev = None
    for k in range(max_iteration + 1):
        assert counts[k] >= 0, f"evaluation {k} was never recorded"
        fit, rmse = statistics(int(counts[k]), float(sums[k]), n)
        if k > 0 and converged(fit, rmse, fit_prev, rmse_prev, relative_fitness, relative_rmse):
            return k
        if k == max_iteration or not can_update(k):
            return k
        fit_prev, rmse_prev = fit, rmse
    raise AssertionError("unreachable")


def margins(src, tgt, T, d):
    """Which rows of Evaluate(T) does fp32 rounding not decide?  -> (nearest [n] int64 in float64, decided [n] bool).

    The kernel's moved point p differs from the exact image of the fp32 R|t by at most e_p per coordinate:
    six roundings (three products, three sums) of terms bounded by a = |r0 x| + |r1 y| + |r2 z| + |t0|, so
    e_p <= 6 EPS32 a (1 + o(1)).  Its fp32 d2 then differs from the exact squared distance D2 to a target by at most
    err = 2 sqrt(3 D2) e_p' + 3 e_p'^2 + 6 EPS32 D2 with e_p' = e_p + EPS32 |dx| (the subtraction rounds once more; |dx| <=
    sqrt(D2)), the last term for the three squares, two sums (and slack).  A row is decided when the gap between its two
    smallest D2 exceeds 2 err (of the larger) and its smallest D2 is further than err from d^2 -- or when every target
    is further than d by more than err (then nothing can be matched).  Exact duplicates of the nearest target (gap 0) are
    never decided."""
    n, m = len(src), len(tgt)
    X = xf32(T).astype(np.float64)
    s64, t64 = src.astype(np.float64), tgt.astype(np.float64)
    p = s64 @ X[:9].reshape(3, 3).T + X[9:]
    a = np.abs(s64) @ np.abs(X[:9].reshape(3, 3)).T + np.abs(X[9:])
    e_p = 6 * EPS32 * a.max(1) * 1.01
    nearest = np.zeros(n, np.int64)
    decided = np.zeros(n, bool)
    thr2 = float(d) * float(d)
    for i0 in range(0, n, 512):
        D2 = ((p[i0:i0 + 512, None, :] - t64[None]) ** 2).sum(2)
        order = np.argsort(D2, 1)[:, :2]
        rows = np.arange(len(D2))
        d0 = D2[rows, order[:, 0]]
        d1 = D2[rows, order[:, 1]] if m > 1 else np.full(len(D2), np.inf)

        def err(v):
            e = e_p[i0:i0 + 512] + EPS32 * np.sqrt(v)
            return 2 * np.sqrt(3 * v) * e + 3 * e * e + 6 * EPS32 * v

        far = d0 - err(d0) > thr2 * (1 + 2 * EPS32)
        clear = (d1 - d0 > 2 * err(np.where(np.isfinite(d1), d1, d0))) & (np.abs(d0 - thr2) > err(d0) + 2 * EPS32 * thr2)
        nearest[i0:i0 + 512] = order[:, 0]
        decided[i0:i0 + 512] = far | clear
    return nearest, decided


def cube_pair(seed, n, m, angle_deg=3.0, shift=0.03, noise=0.0):
    """Seeded clouds, uniform in the unit cube: src [n,3]; tgt [m,3] = the first m source points (cyclically when m > n, then
    jittered so that no two targets coincide) under a rotation of angle_deg about a random axis and a shift, in another
    order -> src, tgt (float32), T_gt [4,4] float64."""
    rng = np.random.RandomState(seed)
    src = rng.rand(n, 3)
    axis = rng.randn(3)
    axis /= np.linalg.norm(axis)
    th = np.radians(angle_deg)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    t = rng.randn(3)
    t *= shift / np.linalg.norm(t)
    base = src[np.arange(m) % max(n, 1)] if n > 0 else rng.rand(m, 3)
    if m > n > 0:
        base = base + rng.randn(m, 3) * 0.01
    c = src.mean(0) if n > 0 else np.zeros(3)
    tgt = (base - c) @ R.T + c + t + rng.randn(m, 3) * noise
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, c + t - R @ c
    return src.astype(np.float32), tgt[rng.permutation(m)].astype(np.float32), T


def lattice_ties(seed, k=6, h=0.125):
    """Planted exact ties: targets on a k x k x k lattice of spacing h (a power of two: every coordinate and distance below
    is exact in fp32) in a random index order, sources at the midpoints of lattice edges along x, so each source has
    exactly two nearest targets at d2 = (h / 2)^2, in different cells of a grid of radius 0.1.
    -> src, tgt (float32), want [n]: the lower of the two target indices."""
    rng = np.random.RandomState(seed)
    ijk = np.stack(np.meshgrid(np.arange(k), np.arange(k), np.arange(k), indexing="ij"), -1).reshape(-1, 3)
    order = rng.permutation(len(ijk))
    tgt = (ijk[order] * h).astype(np.float32)
    index_of = {tuple(c): i for i, c in enumerate(ijk[order].tolist())}
    left = ijk[ijk[:, 0] < k - 1]
    src = ((left + np.array([0.5, 0, 0])) * h).astype(np.float32)
    want = np.array([min(index_of[tuple(c)], index_of[(c[0] + 1, c[1], c[2])]) for c in left.tolist()], np.int64)
    return src, tgt, want
