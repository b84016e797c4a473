"""numpy restatement of the registration back end (include/pcrcg.h "Registration back end"),
stage by stage, for tests/test_registration_*.py.  The product never imports this file."""
import numpy as np

from pcrcg_amd import synthetic

M64 = (1 << 64) - 1
GAMMA = 0x9E3779B97F4A7C15


def splitmix64(x):
    z = (x + GAMMA) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw_rows(seed, h, ransac_n, P):
    rows = []
    for s in range(ransac_n):
        r = splitmix64(((seed << 40) + 8 * h + s) & M64)
        rows.append(((r >> 32) * P) >> 32)
    return rows


def kabsch(ps, pt):
    """float64 fit without scaling, reflection fixed: -> (R, t, singular values descending)."""
    cs, ct = ps.mean(0), pt.mean(0)
    H = (ps - cs).T @ (pt - ct)
    U, S, Vt = np.linalg.svd(H)
    d = np.sign(np.linalg.det(Vt.T @ U.T)) or 1.0
    R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    return R, ct - R @ cs, S


def kabsch_reflects(ps, pt):
    """True when kabsch's reflection fix engages (det(V U^T) < 0) for this sample."""
    H = (ps - ps.mean(0)).T @ (pt - pt.mean(0))
    U, _, Vt = np.linalg.svd(H)
    return bool(np.linalg.det(Vt.T @ U.T) < 0)


def jacobi_fit(ps, pt, dtype=np.longdouble):
    """The fit of csrc/register.hip's hypothesis() restated operation by operation in `dtype` (np.longdouble: the 80-bit
    yardstick of kabsch's own error; np.float64: the kernel's arithmetic): centroids, H, one-sided Jacobi on the columns of
    H (at most 30 sweeps, a pair is skipped when |<h_p, h_q>| <= 1e-17 |h_p| |h_q|), R = v1 u1^T + v2 u2^T +
    (v1 x v2)(u1 x u2)^T, t = ct - R cs -> (R, t, singular values descending, sigma_2 > 1e-12 sigma_1)."""
    ps, pt = np.asarray(ps).astype(dtype), np.asarray(pt).astype(dtype)
    n = len(ps)
    cs, ct = np.zeros(3, dtype), np.zeros(3, dtype)
    for s in range(n):
        cs, ct = cs + ps[s], ct + pt[s]
    cs, ct = cs / dtype(n), ct / dtype(n)
    H = np.zeros((3, 3), dtype)
    for s in range(n):
        H = H + np.outer(ps[s] - cs, pt[s] - ct)
    V = np.eye(3, dtype=dtype)
    for _ in range(30):
        rotated = False
        for p, q in ((0, 1), (0, 2), (1, 2)):
            al = (H[0, p] * H[0, p] + H[1, p] * H[1, p]) + H[2, p] * H[2, p]
            be = (H[0, q] * H[0, q] + H[1, q] * H[1, q]) + H[2, q] * H[2, q]
            ga = (H[0, p] * H[0, q] + H[1, p] * H[1, q]) + H[2, p] * H[2, q]
            if ga == 0 or abs(ga) <= dtype(1e-17) * np.sqrt(al * be):
                continue
            rotated = True
            zeta = (be - al) / (dtype(2) * ga)
            tt = (dtype(1) if zeta >= 0 else dtype(-1)) / (abs(zeta) + np.sqrt(dtype(1) + zeta * zeta))
            cc = dtype(1) / np.sqrt(dtype(1) + tt * tt)
            sn = cc * tt
            for M in (H, V):
                mp, mq = M[:, p].copy(), M[:, q].copy()
                M[:, p] = cc * mp - sn * mq
                M[:, q] = sn * mp + cc * mq
        if not rotated:
            break
    sg = np.sqrt((H[0] * H[0] + H[1] * H[1]) + H[2] * H[2])
    i1 = 0
    for c in (1, 2):
        if sg[c] > sg[i1]:
            i1 = c
    i2 = 1 if i1 == 0 else 0
    for c in range(3):
        if c != i1 and sg[c] > sg[i2]:
            i2 = c
    S = np.array([sg[i1], sg[i2], sg[3 - i1 - i2]])
    if not sg[i2] > dtype(1e-12) * sg[i1]:
        return None, None, S, False
    u1, u2, v1, v2 = H[:, i1] / sg[i1], H[:, i2] / sg[i2], V[:, i1], V[:, i2]
    R = (np.outer(v1, u1) + np.outer(v2, u2)) + np.outer(np.cross(v1, v2), np.cross(u1, u2))
    t = ct - ((R[:, 0] * cs[0] + R[:, 1] * cs[1]) + R[:, 2] * cs[2])
    return R, t, S, True


def kabsch_condition(S, reflects):
    """Condition number of the Kabsch rotation: sigma_1 / (sigma_2 + d sigma_3), d = -1 with the reflection fix."""
    S = [float(x) for x in S]
    gap = S[1] - S[2] if reflects else S[1] + S[2]
    return S[0] / gap if gap > 0 else np.inf


def fit_residual(R, t, ps, pt):
    """float64 sum of |R p_s + t - p_t|^2 over the sample."""
    d = ps.astype(np.float64) @ np.asarray(R, np.float64).T + np.asarray(t, np.float64) - pt.astype(np.float64)
    return float((d * d).sum())


def hypothesis(src, tgt, corr, K, h, ransac_n, thr, sim, dist_check, seed):
    """-> (rows, passed, R, t, margin): margin = the smallest relative distance of a float64 test from its threshold
    (inf when the outcome does not depend on rounding)."""
    rows = draw_rows(seed, h, ransac_n, K)
    if K < ransac_n:
        return rows, False, None, None, np.inf
    sid = corr[rows, 0]
    if len(set(sid.tolist())) < ransac_n:
        return rows, False, None, None, np.inf
    ps = src[sid].astype(np.float64)
    pt = tgt[corr[rows, 1]].astype(np.float64)
    margin = np.inf
    if sim > 0:
        for i in range(ransac_n):
            for j in range(i + 1, ransac_n):
                ds, dt = np.linalg.norm(ps[i] - ps[j]), np.linalg.norm(pt[i] - pt[j])
                scale = max(ds, dt, 1e-300)
                margin = min(margin, abs(ds - dt * sim) / scale, abs(dt - ds * sim) / scale)
                if ds < dt * sim or dt < ds * sim:
                    return rows, False, None, None, margin
    R, t, S = kabsch(ps, pt)
    if S[0] == 0 or not S[1] > 1e-12 * S[0]:
        return rows, False, None, None, margin
    margin = min(margin, abs(S[1] / S[0] - 1e-12))
    if dist_check:
        d = np.linalg.norm(ps @ R.T + t - pt, axis=1)
        margin = min(margin, float(np.min(np.abs(d - thr))) / thr)
        if (d > thr).any():
            return rows, False, R, t, margin
    return rows, True, R, t, margin


def evaluate(src, tgt, xf32, thr):
    """Inlier count and float64 sum of the nearest d2 for the fp32 transform xf32 [12] (R row-major, then t): unfused
    fp32 moves and distances, brute force over the targets."""
    T = np.asarray(xf32, np.float32)
    x, y, z = src[:, 0], src[:, 1], src[:, 2]
    px = ((T[0] * x + T[1] * y) + T[2] * z) + T[9]
    py = ((T[3] * x + T[4] * y) + T[5] * z) + T[10]
    pz = ((T[6] * x + T[7] * y) + T[8] * z) + T[11]
    thr2 = np.float32(float(thr) * float(thr))
    best = np.empty(len(src), np.float32)
    for a in range(0, len(src), 512):
        dx = tgt[None, :, 0] - px[a:a + 512, None]
        dy = tgt[None, :, 1] - py[a:a + 512, None]
        dz = tgt[None, :, 2] - pz[a:a + 512, None]
        best[a:a + 512] = ((dx * dx + dy * dy) + dz * dz).min(1)
    hit = best < thr2
    return int(hit.sum()), float(best[hit].astype(np.float64).sum())


def grid_home_slot(p, thr, tsize):
    """Home slot of the cell of point p in a target hash table of tsize slots, and the cell's key (csrc/cellgrid.h:
    cells of (float)thr * (1 + 1e-5), coordinates biased by 2^20 and packed 21 bits each, mix32, multiply-high)."""
    inv = 1.0 / (float(np.float32(thr)) * (1.0 + 1e-5))
    c = [int(np.floor(float(np.float32(v)) * inv)) + (1 << 20) for v in p]
    key = c[0] | (c[1] << 21) | (c[2] << 42)
    x = key
    x ^= x >> 33
    x = (x * 0xFF51AFD7ED558CCD) & M64
    x ^= x >> 33
    x = (x * 0xC4CEB9FE1A85EC53) & M64
    x ^= x >> 33
    return ((x & 0xFFFFFFFF) * tsize) >> 32, key


def better(a, b):
    """(count, sum, h) ordering of the selection: highest count, then lowest sum, then lowest h."""
    return a[0] > b[0] or (a[0] == b[0] and (a[1] < b[1] or (a[1] == b[1] and a[2] < b[2])))


def select(ids, counts, sums):
    best = None
    for h, c, s in zip(ids, counts, sums):
        if best is None or better((c, s, h), best):
            best = (c, s, h)
    return best


def nn_l2(a, b):
    """float64 nearest neighbour in L2 of every row of a among the rows of b -> (index, relative top-2 gap of the
    score <a, b> - |b|^2 / 2)."""
    a = a.astype(np.float64)
    b = b.astype(np.float64)
    hb = 0.5 * (b * b).sum(1)
    scale = np.linalg.norm(a, axis=1) * np.sqrt(2 * hb.max()) + hb.max()
    idx = np.empty(len(a), np.int64)
    gap = np.full(len(a), np.inf)
    for r in range(0, len(a), 1000):
        s = a[r:r + 1000] @ b.T - hb
        idx[r:r + 1000] = s.argmax(1)
        if s.shape[1] > 1:
            top = -np.partition(-s, 1, axis=1)[:, :2]
            gap[r:r + 1000] = (top[:, 0] - top[:, 1]) / scale[r:r + 1000]
    return idx, gap


def nn_l2_distinct(a, b):
    """nn_l2 with exact duplicate rows of b counted as ONE target: the index is the lowest of the winning row's copies
    (equal rows score the same bits in any arithmetic, so the lowest-index rule decides) and the gap is the one to the
    best DIFFERENT row.  The same as nn_l2 where b has no duplicate rows."""
    ub, first = np.unique(b, axis=0, return_index=True)
    idx, gap = nn_l2(a, ub)
    return first[idx], gap


def mutual_selection(score):
    """The reference's mutual_selection (ref:lib/benchmark_utils.py:270-294) for one [N, M] score: (i, j) with
    j = argmax of row i and i = argmax of column j, first index on ties -> rows, cols in ascending row order."""
    row = score.argmax(1)
    col = score.argmax(0)
    keep = col[row] == np.arange(score.shape[0])
    i = np.nonzero(keep)[0]
    return i, row[i]


def ransac(src, tgt, corr, ransac_n, thr, sim, dist_check, max_iteration, max_validation, seed):
    """The whole back end after matching -> (4x4 float64, fitness, rmse, chosen h or -1)."""
    K = len(corr)
    passing = []
    for h in range(max_iteration):
        _, ok, R, t, _ = hypothesis(src, tgt, corr, K, h, ransac_n, thr, sim, dist_check, seed)
        if ok:
            passing.append((h, R, t))
            if len(passing) == max_validation:
                break
    res = []
    for h, R, t in passing:
        xf = np.concatenate([R.reshape(-1), t]).astype(np.float32)
        c, s = evaluate(src, tgt, xf, thr)
        res.append((c, s, h, R, t))
    T = np.eye(4)
    best = None
    for r in res:
        if best is None or better(r[:3], best[:3]):
            best = r
    if best is None or best[0] == 0:
        return T, 0.0, 0.0, -1
    T[:3, :3], T[:3, 3] = best[3], best[4]
    return T, best[0] / len(src), np.sqrt(best[1] / best[0]), best[2]


def random_rotation(rng):
    q = rng.randn(4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def registration_pair(seed, n=2000, outliers=0.5, c=32, noise=0.003, feat_noise=0.05, shape="shell"):
    """A seeded pair with a known SE(3): tgt = R src + t (+ noise) point for point; descriptors: shared unit vectors
    plus noise, a fraction `outliers` of the source rows replaced by fresh random unit vectors.  shape "shell" is a
    lomatch_pair-style 3DMatch fragment (2 m cube faces), "slab" a KITTI-shaped slab (40 m x 40 m x 0.6 m).
    -> src, tgt, src_feat, tgt_feat, T_gt [4,4] float64."""
    rng = np.random.RandomState(seed)
    if shape == "shell":
        src = synthetic.shell(rng, n, 2.0, 0.02).astype(np.float64)
    else:
        src = rng.rand(n, 3) * np.array([40.0, 40.0, 0.6])
    R = random_rotation(rng)
    t = rng.rand(3) - 0.5
    tgt = src @ R.T + t + rng.randn(n, 3) * noise
    f = rng.randn(n, c)
    f /= np.linalg.norm(f, axis=1, keepdims=True)
    g = f + rng.randn(n, c) * feat_noise
    bad = rng.rand(n) < outliers
    f[bad] = rng.randn(int(bad.sum()), c)
    f = f / np.linalg.norm(f, axis=1, keepdims=True)
    g = g / np.linalg.norm(g, axis=1, keepdims=True)
    perm = rng.permutation(n)                       # the target cloud in another order
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return (src.astype(np.float32), tgt[perm].astype(np.float32), f.astype(np.float32), g[perm].astype(np.float32), T)


def pose_error(T, T_gt):
    """-> (rotation error in degrees, translation error in the same unit as the points)."""
    c = (np.trace(T[:3, :3] @ T_gt[:3, :3].T) - 1) / 2
    return float(np.degrees(np.arccos(np.clip(c, -1, 1)))), float(np.linalg.norm(T[:3, 3] - T_gt[:3, 3]))
